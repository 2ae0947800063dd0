// Device-resident replay storage and sub-trajectory windowing (HBM-bound row copies).
// Reference: surreal/replay/fifo_replay.py:27-48, surreal/replay/uniform_replay.py:36-47,
// surreal/env/exp_sender_wrapper.py:209-264.  The reference keeps Python lists of experience
// dicts and pays pyarrow (de)serialisation around every insert/sample; here each experience field
// is one [capacity, width] fp32 table in HBM and insert/sample are coalesced row copies: one
// wavefront moves one row with 16-byte lanes when the width allows.
#include "smx_common.h"
#include <string.h>

namespace {

#include "smx_synth_env.inc.h"
#include "smx_philox.inc.h"

// copy `n` rows of `width` floats: dst row i <- src row map(i).  A wavefront moves one SEGMENT of
// one row (ROW_SEG floats): a learner batch has few, very wide rows (1024 sub-trajectories of
// 192 KB) and one wave per row left 3/4 of the CUs idle with a single load in flight per lane
// (2.9 TB/s; 5.3 TB/s = the device's copy rate with segments and four loads in flight).
constexpr int ROW_SEG = 2048;             // floats = 8 KB per segment
constexpr int ROW_SEG_BYTES = ROW_SEG * 4;

// Rows are opaque byte strings: `gran` is the widest unit both row pitch and base addresses allow
// (16: float4 lanes, 4: dwords, 1: bytes) -- fp32 fields are rows of 4-byte units, uint8 camera frames
// (3 x 84 x 84 = 21 168 B = 1323 float4) move as what they are instead of being widened to fp32.
template <typename SrcRow, typename DstRow>
__device__ __forceinline__ void copy_rows_bytes_part(const unsigned char* __restrict__ src,
                                                     unsigned char* __restrict__ dst, long n, long row_bytes,
                                                     int gran, SrcRow srow, DstRow drow, long wave, long nwaves);

template <typename SrcRow, typename DstRow>
__device__ __forceinline__ void copy_rows_bytes(const unsigned char* __restrict__ src,
                                                unsigned char* __restrict__ dst, long n, long row_bytes,
                                                int gran, SrcRow srow, DstRow drow) {
    copy_rows_bytes_part(src, dst, n, row_bytes, gran, srow, drow, ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6,
                         ((long)gridDim.x * blockDim.x) >> 6);
}

// the same for the waves [wave, wave + nwaves, ...) of a PART of the grid (several tables gathered by one launch)
template <typename SrcRow, typename DstRow>
__device__ __forceinline__ void copy_rows_bytes_part(const unsigned char* __restrict__ src,
                                                     unsigned char* __restrict__ dst, long n, long row_bytes,
                                                     int gran, SrcRow srow, DstRow drow, long wave, long nwaves) {
    const int lane = threadIdx.x & 63;
    const int nseg = (int)((row_bytes + ROW_SEG_BYTES - 1) / ROW_SEG_BYTES);
    const long items = n * nseg;
    for (long it = wave; it < items; it += nwaves) {
        const long i = it / nseg;
        const long k0 = (it - i * nseg) * (long)ROW_SEG_BYTES;
        const int len = (int)min((long)ROW_SEG_BYTES, row_bytes - k0);
        const unsigned char* s = src + srow(i) * row_bytes + k0;
        unsigned char* d = dst + drow(i) * row_bytes + k0;
        if (gran == 16) {
            const float4* s4 = reinterpret_cast<const float4*>(s);
            float4* d4 = reinterpret_cast<float4*>(d);
            const int n4 = len >> 4;
            int k = lane;
            for (; k + 192 < n4; k += 256) {            // four independent 16-byte loads per lane
                const float4 a = s4[k], b = s4[k + 64], c = s4[k + 128], e = s4[k + 192];
                d4[k] = a; d4[k + 64] = b; d4[k + 128] = c; d4[k + 192] = e;
            }
            for (; k < n4; k += 64) d4[k] = s4[k];
        } else if (gran == 4) {
            const uint32_t* s1 = reinterpret_cast<const uint32_t*>(s);
            uint32_t* d1 = reinterpret_cast<uint32_t*>(d);
            for (int k = lane; k < (len >> 2); k += 64) d1[k] = s1[k];
        } else {
            for (int k = lane; k < len; k += 64) d[k] = s[k];
        }
    }
}

template <typename SrcRow, typename DstRow>
__device__ __forceinline__ void copy_rows(const float* __restrict__ src, float* __restrict__ dst,
                                          long n, int width, bool vec, SrcRow srow, DstRow drow) {
    copy_rows_bytes(reinterpret_cast<const unsigned char*>(src), reinterpret_cast<unsigned char*>(dst), n,
                    (long)width * 4, vec ? 16 : 4, srow, drow);
}

__global__ __launch_bounds__(256) void ring_insert_kernel(float* __restrict__ table, long capacity,
                                                          int width, long cursor,
                                                          const float* __restrict__ src, long n,
                                                          int vec) {
    copy_rows(src, table, n, width, vec != 0, [](long i) { return i; },
              [=](long i) { return (cursor + i) % capacity; });
}

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ table,
                                                          long capacity, int width,
                                                          const int64_t* __restrict__ idx, long n,
                                                          float* __restrict__ dst, int vec) {
    copy_rows(table, dst, n, width, vec != 0,
              [=](long i) {
                  long j = (long)idx[i];
                  j = j < 0 ? 0 : (j >= capacity ? capacity - 1 : j);
                  return j;
              },
              [](long i) { return i; });
}

// the uniform sampler: Philox4x32-10 (smx_philox.inc.h), counter = (offset + i, 0), key = seed
__global__ __launch_bounds__(256) void uniform_indices_kernel(int64_t* __restrict__ idx, long n,
                                                              uint64_t len, uint64_t seed,
                                                              uint64_t offset) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t ctr = offset + (uint64_t)i;
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    // 64 random bits -> [0, len) by 128-bit multiply-high (bias < len / 2^64)
    const uint64_t r64 = ((uint64_t)c[0] << 32) | c[1];
    idx[i] = (int64_t)__umul64hi(r64, len);
}

// the generator by itself, for arbitrary counters and keys: the known-answer self-test (Random123's kat_vectors)
__global__ __launch_bounds__(256) void philox_kat_kernel(const uint32_t* __restrict__ ck, long n, uint32_t* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t c[4] = {ck[6 * i], ck[6 * i + 1], ck[6 * i + 2], ck[6 * i + 3]};
    philox4x32_10(c, ck[6 * i + 4], ck[6 * i + 5]);
    out[4 * i] = c[0]; out[4 * i + 1] = c[1]; out[4 * i + 2] = c[2]; out[4 * i + 3] = c[3];
}

// the noise stream's draws as a tensor: out[k, a, j] = what a launch on N draws for (local actor a, its k-th step, j)
__global__ __launch_bounds__(256) void noise_fill_kernel(smx_noise_stream N, int n, int A, long total, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long ka = i / A;
    const int j = (int)(i - ka * A);
    const int k = (int)(ka / n);
    out[i] = noise_draw(N, ka - (long)k * n, k, j);
}

__device__ __forceinline__ long philox_index(uint64_t ctr, uint64_t len, uint64_t seed) {
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t r64 = ((uint64_t)c[0] << 32) | c[1];
    return (long)__umul64hi(r64, len);
}

// A whole uniform sample in ONE launch (UniformReplay.sample, surreal/replay/uniform_replay.py:36-47): every field's
// table is gathered by its own part of the grid; the row indices are the ones smx_uniform_indices would write (the same
// Philox counters), formed where they are used -- or read from `idx` when the caller injects them.
struct GatherJobs {
    const unsigned char* table[8];
    unsigned char* dst[8];
    long row_bytes[8];
    int gran[8];
    int block0[9];          // first workgroup of each job, [n] = grid size
    int n;
};
__global__ __launch_bounds__(256) void uniform_gather_multi_kernel(GatherJobs J, long capacity, long rows,
                                                                   const int64_t* __restrict__ idx, uint64_t len,
                                                                   uint64_t seed, uint64_t offset,
                                                                   int64_t* __restrict__ idx_out) {
    int j = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) j += (k < J.n && (int)blockIdx.x >= J.block0[k]) ? 1 : 0;
    const long wave = ((long)((int)blockIdx.x - J.block0[j]) * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)(J.block0[j + 1] - J.block0[j]) * blockDim.x) >> 6;
    if (idx_out && j == 0)
        for (long i = (long)((int)blockIdx.x - J.block0[0]) * blockDim.x + threadIdx.x; i < rows;
             i += (long)(J.block0[1] - J.block0[0]) * blockDim.x)
            idx_out[i] = idx ? idx[i] : (int64_t)philox_index(offset + (uint64_t)i, len, seed);
    copy_rows_bytes_part(J.table[j], J.dst[j], rows, J.row_bytes[j], J.gran[j],
                         [=](long i) {
                             long r = idx ? (long)idx[i] : philox_index(offset + (uint64_t)i, len, seed);
                             return r < 0 ? 0 : (r >= capacity ? capacity - 1 : r);
                         },
                         [](long i) { return i; }, wave, nwaves);
}

// The same sample of a frame-pool replay: parts 0 .. J.n - 1 of the grid gather the field tables as above, two more
// build pixel (part J.n) and pixel_next (J.n + 1) for the same rows out of the pool -- item i = (sample row i / S, stack
// position i % S) is one frame of F bytes, moved like a table row: from slot c mod P of the row's actor, c = max(top - S
// + 1 + i % S, frame_first), top = frame_next (pixel: - n_step).  A drawn row is (base + u) % capacity.
struct PoolJobs {
    GatherJobs J;
    unsigned char* pix[2];
    int pgran;
    int pblock0[3];         // first workgroup of the two pool parts, [2] = grid size
    const unsigned char* pool;
    long P, F;
    int actors, S, N;
    const int64_t *frame_next, *frame_first;
    const int* frame_actor;
    long base;
};
__global__ __launch_bounds__(256) void uniform_gather_pool_kernel(PoolJobs Q, long capacity, long rows,
                                                                  const int64_t* __restrict__ idx, uint64_t len,
                                                                  uint64_t seed, uint64_t offset,
                                                                  int64_t* __restrict__ idx_out) {
    const GatherJobs& J = Q.J;
    auto ring = [=](long i) {
        long r = idx ? (long)idx[i] : (Q.base + philox_index(offset + (uint64_t)i, len, seed)) % capacity;
        return r < 0 ? 0 : (r >= capacity ? capacity - 1 : r);
    };
    if ((int)blockIdx.x >= Q.pblock0[0]) {
        const int part = (int)blockIdx.x >= Q.pblock0[1] ? 1 : 0;
        const long wave = ((long)((int)blockIdx.x - Q.pblock0[part]) * blockDim.x + threadIdx.x) >> 6;
        const long nwaves = ((long)(Q.pblock0[part + 1] - Q.pblock0[part]) * blockDim.x) >> 6;
        const int S = Q.S;
        copy_rows_bytes_part(Q.pool, Q.pix[part], rows * S, Q.F, Q.pgran,
                             [=](long i) {
                                 const long r = ring(i / S);
                                 const int k = (int)(i % S);
                                 const long top = (long)Q.frame_next[r] - (part == 0 ? Q.N : 0);
                                 const long lo = (long)Q.frame_first[r];
                                 long c = top - S + 1 + k;
                                 c = c < lo ? lo : c;
                                 int a = Q.frame_actor[r];
                                 a = a < 0 ? 0 : (a >= Q.actors ? Q.actors - 1 : a);
                                 return (long)a * Q.P + ((c % Q.P) + Q.P) % Q.P;
                             },
                             [](long i) { return i; }, wave, nwaves);
        return;
    }
    int j = 0;
#pragma unroll
    for (int k = 1; k < 8; ++k) j += (k < J.n && (int)blockIdx.x >= J.block0[k]) ? 1 : 0;
    const long wave = ((long)((int)blockIdx.x - J.block0[j]) * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)(J.block0[j + 1] - J.block0[j]) * blockDim.x) >> 6;
    if (idx_out && j == 0)
        for (long i = (long)((int)blockIdx.x - J.block0[0]) * blockDim.x + threadIdx.x; i < rows;
             i += (long)(J.block0[1] - J.block0[0]) * blockDim.x)
            idx_out[i] = idx ? idx[i] : (int64_t)((Q.base + philox_index(offset + (uint64_t)i, len, seed)) % capacity);
    copy_rows_bytes_part(J.table[j], J.dst[j], rows, J.row_bytes[j], J.gran[j], ring, [](long i) { return i; }, wave,
                         nwaves);
}

__global__ __launch_bounds__(256) void window_emit_kernel(const float* __restrict__ src, int actors,
                                                          int T, int width, int start, int n_step,
                                                          int stride, int W, float* __restrict__ dst,
                                                          int vec) {
    const long n = (long)actors * W * n_step;
    copy_rows(src, dst, n, width, vec != 0,
              [=](long i) {
                  const long jw = i / n_step;
                  const int j = (int)(i - jw * n_step);
                  const long a = jw / W;
                  const int w = (int)(jw - a * W);
                  return a * T + start + (long)w * stride + j;
              },
              [](long i) { return i; });
}

__global__ __launch_bounds__(256) void ring_insert_bytes_kernel(unsigned char* __restrict__ table, long capacity,
                                                                long row_bytes, long cursor,
                                                                const unsigned char* __restrict__ src, long n,
                                                                int gran) {
    copy_rows_bytes(src, table, n, row_bytes, gran, [](long i) { return i; },
                    [=](long i) { return (cursor + i) % capacity; });
}

__global__ __launch_bounds__(256) void gather_rows_bytes_kernel(const unsigned char* __restrict__ table,
                                                                long capacity, long row_bytes,
                                                                const int64_t* __restrict__ idx, long n,
                                                                unsigned char* __restrict__ dst, int gran) {
    copy_rows_bytes(table, dst, n, row_bytes, gran,
                    [=](long i) {
                        long j = (long)idx[i];
                        j = j < 0 ? 0 : (j >= capacity ? capacity - 1 : j);
                        return j;
                    },
                    [](long i) { return i; });
}

__global__ __launch_bounds__(256) void window_emit_bytes_kernel(const unsigned char* __restrict__ src, int actors,
                                                                int T, long row_bytes, int start, int n_step,
                                                                int stride, int W, unsigned char* __restrict__ dst,
                                                                int gran) {
    const long n = (long)actors * W * n_step;
    copy_rows_bytes(src, dst, n, row_bytes, gran,
                    [=](long i) {
                        const long jw = i / n_step;
                        const int j = (int)(i - jw * n_step);
                        const long a = jw / W;
                        const int w = (int)(jw - a * W);
                        return a * T + start + (long)w * stride + j;
                    },
                    [](long i) { return i; });
}

// "obs stacking" (FrameStackWrapper, surreal/env/wrapper.py:407-472) as index arithmetic over the raw frames of a
// device-resident rollout (one frame per step, row 0 = the frame after reset): the observation of row s is the last
// n_stack frames on the channel axis, oldest first, and a reset fills the history with the first frame --
//   stacked(s)[i] = frames[max(s - (n_stack - 1) + i, first(s))]
// -- cut into W moving windows of n_step rows in the same gather (window_emit's arithmetic).
__global__ __launch_bounds__(256) void frame_stack_kernel(const unsigned char* __restrict__ src, int actors, int R,
                                                          long frame_bytes, int n_stack,
                                                          const int* __restrict__ first, int start, int n_step,
                                                          int stride, int W, unsigned char* __restrict__ dst, int gran) {
    const long n = (long)actors * W * n_step * n_stack;
    copy_rows_bytes(src, dst, n, frame_bytes, gran,
                    [=](long i) {
                        const long q = i / n_stack;
                        const int ii = (int)(i - q * n_stack);
                        const long jw = q / n_step;
                        const int j = (int)(q - jw * n_step);
                        const long a = jw / W;
                        const int w = (int)(jw - a * W);
                        const int sidx = start + w * stride + j;
                        const int lo = first ? first[a * R + sidx] : 0;
                        int f = sidx - (n_stack - 1) + ii;
                        f = f < lo ? lo : f;
                        return a * R + f;
                    },
                    [](long i) { return i; });
}

// the synthetic camera (surreal_amd.env.SyntheticEnv._frame): frame[c, y, x] = (37 c + 5 y + 11 x + 3 t +
// int(100 |s0|)) % 256 for every actor, s0 = the first state component the frame belongs to
__global__ __launch_bounds__(256) void synth_frame_kernel(const float* __restrict__ s0, long ld_s0, int n, int C, int H,
                                                          int Wd, int t, unsigned char* __restrict__ dst, long ld_dst) {
    const long per = (long)C * H * Wd;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * per) return;
    const long a = i / per;
    const int e = (int)(i - a * per);
    const int c = e / (H * Wd), yx = e - c * (H * Wd), y = yx / Wd, x = yx - y * Wd;
    dst[a * ld_dst + e] = synth_frame_px(c, y, x, synth_frame_shift(t, s0[a * ld_s0]));
}

// one thread per (actor, k); the reward needs the whole action row: lanes k < 1 compute it
__global__ __launch_bounds__(256) void synth_env_step_kernel(
    float* __restrict__ state, const float* __restrict__ init_state,
    const float* __restrict__ actions, int n, int D, int A, int t, int episode_len, int slot, int T,
    float* __restrict__ obs_roll, float* __restrict__ act_roll, float* __restrict__ rew_roll,
    float* __restrict__ done_roll, smx_episode_monitor mon) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)n * D) return;
    const long a = i / D;
    const int k = (int)(i - a * D);
    const float s = state[i];
    float ac = actions[a * A + (k % A)];
    ac = fminf(fmaxf(ac, -1.0f), 1.0f);
    const float sn = synth_next(s, ac, synth_drift(k));
    const bool done = (t + 1 >= episode_len);
    if (obs_roll) {
        obs_roll[(a * T + slot) * D + k] = s;
        // the observation AFTER this step (the terminal one when done): obs_next of a window
        // that ends here (exp_sender_wrapper.py:220-221)
        if (slot + 1 < T) obs_roll[(a * T + slot + 1) * D + k] = sn;
    }
    if (k < A && act_roll) {
        float av = actions[a * A + k];
        act_roll[(a * T + slot) * A + k] = fminf(fmaxf(av, -1.0f), 1.0f);
    }
    if (k == 0) {
        double q = 0.0;
        for (int j = 0; j < A; ++j) {
            float av = fminf(fmaxf(actions[a * A + j], -1.0f), 1.0f);
            q += (double)av * (double)av;
        }
        const float rew = synth_reward(q, sn);
        if (rew_roll) rew_roll[a * T + slot] = rew;
        if (done_roll) done_roll[a * T + slot] = done ? 1.0f : 0.0f;
        if (mon.ep_reward) episode_account(mon, a, rew, done);
    }
    state[i] = done ? init_state[i] : sn;
}

// The same launch on SMX_TASK_REACH (reach_* of smx_synth_env.inc.h): an actor's elements are coupled, so ONE thread
// steps the whole row of actor a, mass by mass -- every value it reads it reads before it writes it, no two threads
// touch the same row.  (The device's own one-step reference and the evaluation's step: not a hot path.)
__global__ __launch_bounds__(256) void reach_env_step_kernel(
    float* __restrict__ state, const float* __restrict__ init_state,
    const float* __restrict__ actions, int n, int D, int A, int t, int episode_len, int slot, int T,
    float* __restrict__ obs_roll, float* __restrict__ act_roll, float* __restrict__ rew_roll,
    float* __restrict__ done_roll, smx_episode_monitor mon, smx_reset_stream R) {
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const bool done = (t + 1 >= episode_len);
    const bool draw = done && R.enabled;             // the reset row from the stream (reach_reset_value), not init_state
    const float dsc = reset_disturbance(R);          // 0: no disturbance; else step t of episode R.episode - 1 draws w[j]
    float* s = state + a * D;
    const float* s0 = init_state + a * D;
    float* orow = obs_roll ? obs_roll + (a * T + slot) * D : nullptr;
    const bool onext = orow && slot + 1 < T;         // the observation AFTER this step (synth_env_step_kernel)
    double sd = 0.0, sa = 0.0;
    for (int j = 0; j < A; ++j) {
        const float ac = fminf(fmaxf(actions[a * A + j], -1.0f), 1.0f);
        const float p = s[j], v = s[A + j], g = s[2 * A + j];
        float sw = 0.f;
        if (dsc != 0.0f)
            sw = dsc * disturbance_uniform(R.seed, (uint32_t)(R.actor_base + a), (uint32_t)(R.episode - 1), (uint32_t)t, j);
        const float vn = reach_next_v(v, ac, dsc != 0.0f, sw);
        const float pn = reach_next_p(p, vn);
        const float d = pn - g;
        sd += (double)d * (double)d;
        if (orow) {
            orow[j] = p; orow[A + j] = v; orow[2 * A + j] = g;
            if (onext) { orow[D + j] = pn; orow[D + A + j] = vn; orow[D + 2 * A + j] = g; }
        }
        if (act_roll) act_roll[(a * T + slot) * A + j] = ac;
        if (draw) {
            s[j] = reach_reset_value(R, a, 0, j, A);
            s[A + j] = reach_reset_value(R, a, 0, A + j, A);
            s[2 * A + j] = reach_reset_value(R, a, 0, 2 * A + j, A);
        } else {
            s[j] = done ? s0[j] : pn;
            s[A + j] = done ? s0[A + j] : vn;
            s[2 * A + j] = done ? s0[2 * A + j] : g;
        }
    }
    for (int j = 0; j < A; ++j) {
        const float ac = fminf(fmaxf(actions[a * A + j], -1.0f), 1.0f);
        sa += (double)ac * (double)ac;
    }
    const float rew = reach_reward(sd, sa);
    if (rew_roll) rew_roll[a * T + slot] = rew;
    if (done_roll) done_roll[a * T + slot] = done ? 1.0f : 0.0f;
    if (mon.ep_reward) episode_account(mon, a, rew, done);
}

// The same launch on SMX_TASK_ARM (arm_* of smx_synth_env.inc.h): ONE thread steps the whole row of actor a, link by link,
// as reach_env_step_kernel does -- the goal is read before anything is written, no two threads touch the same row.
__global__ __launch_bounds__(256) void arm_env_step_kernel(
    float* __restrict__ state, const float* __restrict__ init_state,
    const float* __restrict__ actions, int n, int D, int A, int t, int episode_len, int slot, int T,
    float* __restrict__ obs_roll, float* __restrict__ act_roll, float* __restrict__ rew_roll,
    float* __restrict__ done_roll, smx_episode_monitor mon, smx_reset_stream R) {
    const long a = (long)blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const bool done = (t + 1 >= episode_len);
    const bool draw = done && R.enabled;             // the reset row from the stream (arm_reset_value), not init_state
    const float dsc = reset_disturbance(R);          // 0: no disturbance; else step t of episode R.episode - 1 draws w[j]
    float* s = state + a * D;
    const float* s0 = init_state + a * D;
    float* orow = obs_roll ? obs_roll + (a * T + slot) * D : nullptr;
    const bool onext = orow && slot + 1 < T;         // the observation AFTER this step (synth_env_step_kernel)
    const float g0 = s[2 * A], g1 = s[2 * A + 1];
    double sx = 0.0, sy = 0.0, sa = 0.0;
    for (int j = 0; j < A; ++j) {
        const float ac = fminf(fmaxf(actions[a * A + j], -1.0f), 1.0f);
        const float th = s[j], om = s[A + j];
        float sw = 0.f;
        if (dsc != 0.0f)
            sw = dsc * disturbance_uniform(R.seed, (uint32_t)(R.actor_base + a), (uint32_t)(R.episode - 1), (uint32_t)t, j);
        const float on = arm_next_omega(om, ac, dsc != 0.0f, sw);
        const float tn = arm_next_theta(th, on);
        float sn, cs;
        arm_sincos(tn, sn, cs);
        sx += (double)cs;
        sy += (double)sn;
        if (orow) {
            orow[j] = th; orow[A + j] = om;
            if (onext) { orow[D + j] = tn; orow[D + A + j] = on; }
        }
        if (act_roll) act_roll[(a * T + slot) * A + j] = ac;
        if (draw) {
            s[j] = arm_reset_value(R, a, 0, j, A);
            s[A + j] = arm_reset_value(R, a, 0, A + j, A);
        } else {
            s[j] = done ? s0[j] : tn;
            s[A + j] = done ? s0[A + j] : on;
        }
    }
    for (int i = 0; i < 2; ++i) {
        const float g = i ? g1 : g0;
        if (orow) {
            orow[2 * A + i] = g;
            if (onext) orow[D + 2 * A + i] = g;
        }
        s[2 * A + i] = draw ? arm_reset_value(R, a, 0, 2 * A + i, A) : (done ? s0[2 * A + i] : g);
    }
    for (int j = 0; j < A; ++j) {
        const float ac = fminf(fmaxf(actions[a * A + j], -1.0f), 1.0f);
        sa += (double)ac * (double)ac;
    }
    const float rew = arm_reward(sx, sy, sa, arm_link(A), g0, g1);
    if (rew_roll) rew_roll[a * T + slot] = rew;
    if (done_roll) done_roll[a * T + slot] = done ? 1.0f : 0.0f;
    if (mon.ep_reward) episode_account(mon, a, rew, done);
}

// out [n, D] <- the rows the actors of a reach env begin episode R.episode with (smx_reset_fill_f32): one thread per element
__global__ __launch_bounds__(256) void reset_fill_kernel(smx_reset_stream R, int D, long total, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    out[i] = reach_reset_value(R, i / D, 0, (int)(i % D), D / 3);
}
// the same of an arm env (D = 2 J + 2)
__global__ __launch_bounds__(256) void arm_reset_fill_kernel(smx_reset_stream R, int D, long total, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    out[i] = arm_reset_value(R, i / D, 0, (int)(i % D), (D - 2) / 2);
}

// The acting head, the environment step and the next observation's z-filter in one launch -- the
// glue between two policy forwards of a device-resident rollout (sampling head as
// smx_diaggauss_sample_f32, dynamics as synth_env_step_kernel, filter as
// smx_zfilter_forward_sums_f32: same expressions, same results).
__global__ __launch_bounds__(256) void synth_act_env_step_kernel(smx_synth_act_step_t p) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int D = p.D, A = p.A, T = p.T, slot = p.slot;
    if (i >= (long)p.n * D) return;
    const long a = i / D;
    const int k = (int)(i - a * D);
    const float nz = p.noise_scale ? p.noise_scale[a] : 1.0f;
    const bool noisy = noise_on(p.eps, p.noise);
    auto action = [&](int j, float& mu, float& sd) {
        mu = p.mean[a * p.ld_mean + j];
        sd = expf(p.log_var[j]);
        if (p.noise_scale) sd = sd * nz;
        float act = noisy ? noise_pick(p.eps, a * p.ld_eps + j, p.noise, a, 0, j) * sd + mu : mu;
        if (act == act) act = fminf(fmaxf(act, -1.0f), 1.0f);
        return act;
    };
    float mu, sd;
    const float ac = action(k % A, mu, sd);
    const float s = p.state[i];
    const float sn = synth_next(s, ac, synth_drift(k));
    const bool done = (p.t + 1 >= p.episode_len);
    if (p.obs_roll) {
        p.obs_roll[(a * T + slot) * D + k] = s;
        if (slot + 1 < T) p.obs_roll[(a * T + slot + 1) * D + k] = sn;
    }
    if (k < A) {                                      // here k % A == k
        if (p.act_roll) p.act_roll[(a * T + slot) * A + k] = ac;
        if (p.pd_roll) {
            p.pd_roll[(a * T + slot) * 2 * A + k] = mu;
            p.pd_roll[(a * T + slot) * 2 * A + A + k] = sd;
        }
    }
    if (k == 0) {
        double q = 0.0;
        for (int j = 0; j < A; ++j) {
            float m2, s2;
            const float av = action(j, m2, s2);
            q += (double)av * (double)av;
        }
        const float rew = synth_reward(q, sn);
        if (p.rew_roll) p.rew_roll[a * T + slot] = rew;
        if (p.done_roll) p.done_roll[a * T + slot] = done ? 1.0f : 0.0f;
        if (p.mon.ep_reward) episode_account(p.mon, a, rew, done);
    }
    const float next = done ? p.init_state[i] : sn;
    p.state[i] = next;
    if (p.xn_out) {
        float z = next;
        if (p.zsum) {
            float m, sz;
            zfilter_stats(p.zsum, p.zsumsq, p.zcount, p.zeps, k, m, sz);
            z = zclamp(next, m, sz);
        }
        p.xn_out[i] = z;
    }
}

// The same step with the policy's OUTPUT LAYER folded in: one workgroup per actor forms mean = act(h2 . W3^T + b3)
// itself (A <= 32 outputs, eight lanes per output, a fixed-order tree) and goes on as synth_act_env_step_kernel does --
// an acting step is then three dependent launches (hidden layer 1, hidden layer 2, this) instead of four.
__global__ __launch_bounds__(256) void synth_act_head_step_kernel(smx_synth_act_step_t p, const float* __restrict__ W3,
                                                                  const float* __restrict__ b3,
                                                                  const float* __restrict__ h2, long ld_h2, int H2,
                                                                  int out_act) {
    __shared__ float s_act[32];
    const int tid = threadIdx.x;
    const long a = blockIdx.x;
    const int D = p.D, A = p.A, T = p.T, slot = p.slot;
    {
        const int j = tid >> 3, l = tid & 7;
        float acc = 0.f;
        if (j < A) {
            const float* hr = h2 + a * ld_h2;
            const float* wr = W3 + (size_t)j * H2;
            for (int k = l; k < H2; k += 8) acc = fmaf(hr[k], wr[k], acc);
        }
        acc += __shfl_xor(acc, 1, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 4, 64);
        if (j < A && l == 0) {
            float mu = acc + b3[j];
            if (out_act == SMX_ACT_TANH) mu = tanhf(mu);
            else if (out_act == SMX_ACT_RELU) mu = mu < 0.f ? 0.f : mu;
            const float nz = p.noise_scale ? p.noise_scale[a] : 1.0f;
            float sd = expf(p.log_var[j]);
            if (p.noise_scale) sd = sd * nz;
            float act = noise_on(p.eps, p.noise) ? noise_pick(p.eps, a * p.ld_eps + j, p.noise, a, 0, j) * sd + mu : mu;
            if (act == act) act = fminf(fmaxf(act, -1.0f), 1.0f);
            s_act[j] = act;
            if (p.act_roll) p.act_roll[(a * T + slot) * A + j] = act;
            if (p.pd_roll) {
                p.pd_roll[(a * T + slot) * 2 * A + j] = mu;
                p.pd_roll[(a * T + slot) * 2 * A + A + j] = sd;
            }
        }
    }
    __syncthreads();
    const bool done = (p.t + 1 >= p.episode_len);
    for (int k = tid; k < D; k += 256) {
        const long i = a * D + k;
        const float ac = s_act[k % A];
        const float s = p.state[i];
        const float sn = synth_next(s, ac, synth_drift(k));
        if (p.obs_roll) {
            p.obs_roll[(a * T + slot) * D + k] = s;
            if (slot + 1 < T) p.obs_roll[(a * T + slot + 1) * D + k] = sn;
        }
        if (k == 0) {
            double q = 0.0;
            for (int j = 0; j < A; ++j) q += (double)s_act[j] * (double)s_act[j];
            const float rew = synth_reward(q, sn);
            if (p.rew_roll) p.rew_roll[a * T + slot] = rew;
            if (p.done_roll) p.done_roll[a * T + slot] = done ? 1.0f : 0.0f;
            if (p.mon.ep_reward) episode_account(p.mon, a, rew, done);
        }
        const float next = done ? p.init_state[i] : sn;
        p.state[i] = next;
        if (p.xn_out) {
            float z = next;
            if (p.zsum) {
                float m, sz;
                zfilter_stats(p.zsum, p.zsumsq, p.zcount, p.zeps, k, m, sz);
                z = zclamp(next, m, sz);
            }
            p.xn_out[i] = z;
        }
    }
}

inline unsigned row_blocks(long n, int width) {
    const long items = n * ((width + ROW_SEG - 1) / ROW_SEG);
    long b = (items + 3) / 4;  // 4 waves (row segments) per block
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

inline int can_vec(const void* a, const void* b, int width) {
    return (width % 4 == 0) && ((((uintptr_t)a | (uintptr_t)b) & 15) == 0);
}

inline unsigned row_blocks_bytes(long n, long row_bytes) {
    const long items = n * ((row_bytes + ROW_SEG_BYTES - 1) / ROW_SEG_BYTES);
    long b = (items + 3) / 4;
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (unsigned)b;
}

inline int byte_gran(const void* a, const void* b, long row_bytes) {
    const uintptr_t u = (uintptr_t)a | (uintptr_t)b | (uintptr_t)row_bytes;
    return (u & 15) == 0 ? 16 : ((u & 3) == 0 ? 4 : 1);
}

// the field tables of a one-launch sample -> J, their workgroups counted from `base` on
int gather_jobs(const smx_gather_job_t* jobs, int njobs, int64_t rows, GatherJobs& J, int& base) {
    J.n = njobs;
    for (int k = 0; k < njobs; ++k) {
        SMX_REQUIRE(jobs[k].table && jobs[k].dst, SMX_E_NULL);
        SMX_REQUIRE(jobs[k].row_bytes > 0, SMX_E_SHAPE);
        J.table[k] = (const unsigned char*)jobs[k].table;
        J.dst[k] = (unsigned char*)jobs[k].dst;
        J.row_bytes[k] = (long)jobs[k].row_bytes;
        J.gran[k] = byte_gran(jobs[k].table, jobs[k].dst, (long)jobs[k].row_bytes);
        J.block0[k] = base;
        base += (int)row_blocks_bytes((long)rows, (long)jobs[k].row_bytes);
    }
    for (int k = njobs; k <= 8; ++k) J.block0[k] = base;
    return SMX_OK;
}

}  // namespace

extern "C" int smx_ring_insert_f32(float* table, int64_t capacity, int32_t width, int64_t cursor,
                                   const float* src, int64_t n, smx_stream_t stream) {
    SMX_REQUIRE(table && src, SMX_E_NULL);
    SMX_REQUIRE(capacity > 0 && width > 0 && cursor >= 0 && cursor < capacity && n > 0 &&
                    n <= capacity, SMX_E_SHAPE);
    hipLaunchKernelGGL(ring_insert_kernel, dim3(row_blocks(n, width)), dim3(256), 0, smx_s(stream), table,
                       (long)capacity, width, (long)cursor, src, (long)n, can_vec(table, src, width));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_gather_rows_f32(const float* table, int64_t capacity, int32_t width,
                                   const int64_t* idx, int64_t n, float* dst, smx_stream_t stream) {
    SMX_REQUIRE(table && idx && dst, SMX_E_NULL);
    SMX_REQUIRE(capacity > 0 && width > 0 && n > 0, SMX_E_SHAPE);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(row_blocks(n, width)), dim3(256), 0, smx_s(stream), table,
                       (long)capacity, width, idx, (long)n, dst, can_vec(table, dst, width));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_philox4x32_10(const uint32_t* ctr_key, int64_t n, uint32_t* out, smx_stream_t stream) {
    SMX_REQUIRE(ctr_key && out, SMX_E_NULL);
    SMX_REQUIRE(n > 0, SMX_E_SHAPE);
    hipLaunchKernelGGL(philox_kat_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, smx_s(stream), ctr_key, (long)n, out);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_noise_fill_f32(const struct smx_noise_stream* noise, int32_t steps, int32_t n, int32_t A, float* out,
                                  smx_stream_t stream) {
    SMX_REQUIRE(noise && out, SMX_E_NULL);
    smx_noise_stream N = *noise;
    N.enabled = 1;
    SMX_REQUIRE(steps > 0 && n > 0 && A > 0 && noise_shape_ok(N, n), SMX_E_SHAPE);
    const long total = (long)steps * n * A;
    SMX_REQUIRE((total + 255) / 256 <= 0x7fffffffL, SMX_E_SHAPE);
    hipLaunchKernelGGL(noise_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, smx_s(stream), N, n, A, total,
                       out);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_uniform_indices(int64_t* idx, int64_t n, int64_t len, uint64_t seed,
                                   uint64_t offset, smx_stream_t stream) {
    SMX_REQUIRE(idx, SMX_E_NULL);
    SMX_REQUIRE(n > 0 && len > 0, SMX_E_SHAPE);
    hipLaunchKernelGGL(uniform_indices_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       smx_s(stream), idx, (long)n, (uint64_t)len, seed, offset);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_uniform_gather_multi(const smx_gather_job_t* jobs, int32_t njobs, int64_t capacity, int64_t rows,
                                        const int64_t* idx, int64_t len, uint64_t seed, uint64_t offset,
                                        int64_t* idx_out, smx_stream_t stream) {
    SMX_REQUIRE(jobs, SMX_E_NULL);
    SMX_REQUIRE(njobs >= 1 && njobs <= 8 && capacity > 0 && rows > 0 && (idx || (len > 0 && len <= capacity)), SMX_E_SHAPE);
    GatherJobs J;
    int base = 0;
    const int rc = gather_jobs(jobs, njobs, rows, J, base);
    if (rc != SMX_OK) return rc;
    hipLaunchKernelGGL(uniform_gather_multi_kernel, dim3((unsigned)base), dim3(256), 0, smx_s(stream), J, (long)capacity,
                       (long)rows, idx, (uint64_t)len, seed, offset, idx_out);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_uniform_gather_pool(const smx_gather_job_t* jobs, int32_t njobs, const struct smx_gather_pool* pool,
                                       int64_t capacity, int64_t rows, const int64_t* idx, int64_t len, uint64_t seed,
                                       uint64_t offset, int64_t* idx_out, smx_stream_t stream) {
    SMX_REQUIRE(jobs && pool, SMX_E_NULL);
    SMX_REQUIRE(pool->pool && pool->frame_next && pool->frame_first && pool->frame_actor && pool->pixel && pool->pixel_next,
                SMX_E_NULL);
    SMX_REQUIRE(njobs >= 1 && njobs <= 8 && capacity > 0 && rows > 0 && (idx || (len > 0 && len <= capacity)), SMX_E_SHAPE);
    const int S = pool->frame_stacks;
    SMX_REQUIRE(pool->actors > 0 && S > 0 && pool->n_step > 0 && pool->frame_bytes > 0, SMX_E_SHAPE);
    SMX_REQUIRE(pool->pool_len >= (int64_t)pool->n_step + S + 1 && pool->base >= 0 && pool->base < capacity, SMX_E_SHAPE);
    SMX_REQUIRE((((uintptr_t)pool->frame_next | (uintptr_t)pool->frame_first) & 7) == 0 &&
                ((uintptr_t)pool->frame_actor & 3) == 0, SMX_E_ALIGN);
    PoolJobs Q;
    int base = 0;
    const int rc = gather_jobs(jobs, njobs, rows, Q.J, base);
    if (rc != SMX_OK) return rc;
    Q.pix[0] = pool->pixel; Q.pix[1] = pool->pixel_next;
    Q.pool = pool->pool; Q.P = (long)pool->pool_len; Q.F = (long)pool->frame_bytes;
    Q.actors = pool->actors; Q.S = S; Q.N = pool->n_step;
    Q.frame_next = pool->frame_next; Q.frame_first = pool->frame_first; Q.frame_actor = pool->frame_actor;
    Q.base = (long)pool->base;
    // one unit for both parts: 16 bytes where the frame size, the pool and both destinations allow (4, else 1)
    const int g0 = byte_gran(pool->pool, pool->pixel, Q.F), g1 = byte_gran(pool->pool, pool->pixel_next, Q.F);
    Q.pgran = g0 < g1 ? g0 : g1;
    for (int part = 0; part < 2; ++part) {
        Q.pblock0[part] = base;
        base += (int)row_blocks_bytes((long)rows * S, Q.F);
    }
    Q.pblock0[2] = base;
    hipLaunchKernelGGL(uniform_gather_pool_kernel, dim3((unsigned)base), dim3(256), 0, smx_s(stream), Q, (long)capacity,
                       (long)rows, idx, (uint64_t)len, seed, offset, idx_out);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_window_emit_f32(const float* src, int32_t actors, int32_t T, int32_t width,
                                   int32_t start, int32_t n_step, int32_t stride, int32_t W,
                                   float* dst, smx_stream_t stream) {
    SMX_REQUIRE(src && dst, SMX_E_NULL);
    SMX_REQUIRE(actors > 0 && T > 0 && width > 0 && n_step > 0 && stride > 0 && W > 0 && start >= 0 &&
                    start + (long)(W - 1) * stride + n_step <= T, SMX_E_SHAPE);
    const long n = (long)actors * W * n_step;
    hipLaunchKernelGGL(window_emit_kernel, dim3(row_blocks(n, width)), dim3(256), 0, smx_s(stream), src,
                       actors, T, width, start, n_step, stride, W, dst, can_vec(src, dst, width));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_ring_insert_bytes(void* table, int64_t capacity, int64_t row_bytes, int64_t cursor,
                                     const void* src, int64_t n, smx_stream_t stream) {
    SMX_REQUIRE(table && src, SMX_E_NULL);
    SMX_REQUIRE(capacity > 0 && row_bytes > 0 && cursor >= 0 && cursor < capacity && n > 0 && n <= capacity,
                SMX_E_SHAPE);
    hipLaunchKernelGGL(ring_insert_bytes_kernel, dim3(row_blocks_bytes(n, row_bytes)), dim3(256), 0, smx_s(stream),
                       (unsigned char*)table, (long)capacity, (long)row_bytes, (long)cursor,
                       (const unsigned char*)src, (long)n, byte_gran(table, src, row_bytes));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_gather_rows_bytes(const void* table, int64_t capacity, int64_t row_bytes, const int64_t* idx,
                                     int64_t n, void* dst, smx_stream_t stream) {
    SMX_REQUIRE(table && idx && dst, SMX_E_NULL);
    SMX_REQUIRE(capacity > 0 && row_bytes > 0 && n > 0, SMX_E_SHAPE);
    hipLaunchKernelGGL(gather_rows_bytes_kernel, dim3(row_blocks_bytes(n, row_bytes)), dim3(256), 0, smx_s(stream),
                       (const unsigned char*)table, (long)capacity, (long)row_bytes, idx, (long)n,
                       (unsigned char*)dst, byte_gran(table, dst, row_bytes));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_window_emit_bytes(const void* src, int32_t actors, int32_t T, int64_t row_bytes, int32_t start,
                                     int32_t n_step, int32_t stride, int32_t W, void* dst, smx_stream_t stream) {
    SMX_REQUIRE(src && dst, SMX_E_NULL);
    SMX_REQUIRE(actors > 0 && T > 0 && row_bytes > 0 && n_step > 0 && stride > 0 && W > 0 && start >= 0 &&
                    start + (long)(W - 1) * stride + n_step <= T, SMX_E_SHAPE);
    const long n = (long)actors * W * n_step;
    hipLaunchKernelGGL(window_emit_bytes_kernel, dim3(row_blocks_bytes(n, row_bytes)), dim3(256), 0, smx_s(stream),
                       (const unsigned char*)src, actors, T, (long)row_bytes, start, n_step, stride, W,
                       (unsigned char*)dst, byte_gran(src, dst, row_bytes));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_frame_stack_u8(const void* frames, int32_t actors, int32_t R, int64_t frame_bytes, int32_t n_stack,
                                  const int32_t* episode_first, int32_t start, int32_t n_step, int32_t stride, int32_t W,
                                  void* dst, smx_stream_t stream) {
    SMX_REQUIRE(frames && dst, SMX_E_NULL);
    SMX_REQUIRE(actors > 0 && R > 0 && frame_bytes > 0 && n_stack > 0 && n_step > 0 && stride > 0 && W > 0 && start >= 0 &&
                    start + (long)(W - 1) * stride + n_step <= R, SMX_E_SHAPE);
    const long n = (long)actors * W * n_step * n_stack;
    hipLaunchKernelGGL(frame_stack_kernel, dim3(row_blocks_bytes(n, frame_bytes)), dim3(256), 0, smx_s(stream),
                       (const unsigned char*)frames, actors, R, (long)frame_bytes, n_stack, (const int*)episode_first, start,
                       n_step, stride, W, (unsigned char*)dst, byte_gran(frames, dst, frame_bytes));
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_frame_u8(const float* s0, int64_t ld_s0, int32_t n, int32_t C, int32_t H, int32_t W, int32_t t,
                                  void* dst, int64_t ld_dst, smx_stream_t stream) {
    SMX_REQUIRE(s0 && dst, SMX_E_NULL);
    SMX_REQUIRE(n > 0 && C > 0 && H > 0 && W > 0 && t >= 0 && ld_s0 > 0 && ld_dst >= (int64_t)C * H * W, SMX_E_SHAPE);
    const long total = (long)n * C * H * W;
    hipLaunchKernelGGL(synth_frame_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, smx_s(stream), s0,
                       (long)ld_s0, n, C, H, W, t, (unsigned char*)dst, (long)ld_dst);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_act_env_step_f32(const smx_synth_act_step_t* args, smx_stream_t stream) {
    SMX_REQUIRE(args, SMX_E_NULL);
    const smx_synth_act_step_t& p = *args;
    SMX_REQUIRE(p.state && p.init_state && p.mean && p.log_var, SMX_E_NULL);
    SMX_REQUIRE(p.n > 0 && p.D > 0 && p.A > 0 && p.A <= p.D && p.T > 0 && p.slot >= 0 && p.slot < p.T &&
                    p.episode_len > 0 && p.ld_mean >= p.A && (!p.eps || p.ld_eps >= p.A), SMX_E_SHAPE);
    SMX_REQUIRE(!p.zsum || (p.zsumsq && p.zcount && p.xn_out), SMX_E_NULL);
    SMX_REQUIRE(episode_pointers_ok(p.mon), SMX_E_NULL);
    SMX_REQUIRE(episode_shape_ok(p.mon) && noise_shape_ok(p.noise, p.n), SMX_E_SHAPE);
    const long total = (long)p.n * p.D;
    hipLaunchKernelGGL(synth_act_env_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       smx_s(stream), p);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_act_env_step_head_f32(const smx_synth_act_step_t* args, const float* W3, const float* b3,
                                               const float* h2, int64_t ld_h2, int32_t H2, int32_t out_act,
                                               smx_stream_t stream) {
    SMX_REQUIRE(args && W3 && b3 && h2, SMX_E_NULL);
    const smx_synth_act_step_t& p = *args;
    SMX_REQUIRE(p.state && p.init_state && p.log_var, SMX_E_NULL);
    SMX_REQUIRE(p.n > 0 && p.D > 0 && p.A > 0 && p.A <= 32 && p.A <= p.D && p.T > 0 && p.slot >= 0 && p.slot < p.T &&
                    p.episode_len > 0 && H2 > 0 && ld_h2 >= H2 && (!p.eps || p.ld_eps >= p.A), SMX_E_SHAPE);
    SMX_REQUIRE(!p.zsum || (p.zsumsq && p.zcount && p.xn_out), SMX_E_NULL);
    SMX_REQUIRE(episode_pointers_ok(p.mon), SMX_E_NULL);
    SMX_REQUIRE(episode_shape_ok(p.mon) && noise_shape_ok(p.noise, p.n), SMX_E_SHAPE);
    hipLaunchKernelGGL(synth_act_head_step_kernel, dim3((unsigned)p.n), dim3(256), 0, smx_s(stream), p, W3, b3, h2,
                       (long)ld_h2, H2, out_act);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_env_step_f32(float* state, const float* init_state, const float* actions,
                                      int32_t n, int32_t D, int32_t A, int32_t t,
                                      int32_t episode_len, int32_t slot, int32_t T, float* obs_roll,
                                      float* act_roll, float* rew_roll, float* done_roll,
                                      const struct smx_episode_monitor* mon, smx_stream_t stream) {
    SMX_REQUIRE(state && init_state && actions, SMX_E_NULL);
    SMX_REQUIRE(n > 0 && D > 0 && A > 0 && A <= D && T > 0 && slot >= 0 && slot < T && episode_len > 0,
                SMX_E_SHAPE);
    smx_episode_monitor M;
    memset(&M, 0, sizeof(M));
    if (mon) M = *mon;
    SMX_REQUIRE(episode_pointers_ok(M), SMX_E_NULL);
    SMX_REQUIRE(episode_shape_ok(M), SMX_E_SHAPE);
    const long total = (long)n * D;
    hipLaunchKernelGGL(synth_env_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       smx_s(stream), state, init_state, actions, n, D, A, t, episode_len, slot, T,
                       obs_roll, act_roll, rew_roll, done_roll, M);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

// the task entry point, with the reset stream or (null: none, or a disabled one) without
static int synth_task_env_step(float* state, const float* init_state, const float* actions, int32_t n, int32_t D, int32_t A,
                               int32_t t, int32_t episode_len, int32_t slot, int32_t T, float* obs_roll, float* act_roll,
                               float* rew_roll, float* done_roll, const struct smx_episode_monitor* mon, int32_t task,
                               const smx_reset_stream* resets, smx_stream_t stream) {
    SMX_REQUIRE(!(resets && task == SMX_TASK_DRIFT), SMX_E_UNSUPPORTED);
    if (task == SMX_TASK_DRIFT)
        return smx_synth_env_step_f32(state, init_state, actions, n, D, A, t, episode_len, slot, T, obs_roll, act_roll,
                                      rew_roll, done_roll, mon, stream);
    SMX_REQUIRE((task == SMX_TASK_REACH || task == SMX_TASK_ARM) && synth_task_ok(task, D, A), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(state && init_state && actions, SMX_E_NULL);
    SMX_REQUIRE(n > 0 && T > 0 && slot >= 0 && slot < T && episode_len > 0, SMX_E_SHAPE);
    smx_episode_monitor M;
    memset(&M, 0, sizeof(M));
    if (mon) M = *mon;
    SMX_REQUIRE(episode_pointers_ok(M), SMX_E_NULL);
    SMX_REQUIRE(episode_shape_ok(M), SMX_E_SHAPE);
    smx_reset_stream R;
    memset(&R, 0, sizeof(R));
    if (resets) R = *resets;
    SMX_REQUIRE(reset_shape_ok(R, n), SMX_E_SHAPE);
    // (a disturbed step: its episode R.episode - 1 and its step t within it are counter words)
    SMX_REQUIRE(disturbance_rollout_ok(R, 0, 1, 1) && (reset_disturbance(R) == 0.0f || (t >= 0 && t < episode_len)), SMX_E_SHAPE);
    hipLaunchKernelGGL(task == SMX_TASK_ARM ? arm_env_step_kernel : reach_env_step_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, smx_s(stream), state, init_state, actions, n, D, A, t, episode_len, slot, T, obs_roll,
                       act_roll, rew_roll, done_roll, M, R);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_synth_task_env_step_f32(float* state, const float* init_state, const float* actions,
                                           int32_t n, int32_t D, int32_t A, int32_t t,
                                           int32_t episode_len, int32_t slot, int32_t T, float* obs_roll,
                                           float* act_roll, float* rew_roll, float* done_roll,
                                           const struct smx_episode_monitor* mon, int32_t task, smx_stream_t stream) {
    return synth_task_env_step(state, init_state, actions, n, D, A, t, episode_len, slot, T, obs_roll, act_roll, rew_roll,
                               done_roll, mon, task, nullptr, stream);
}

extern "C" int smx_synth_task_env_step_resets_f32(float* state, const float* init_state, const float* actions,
                                                  int32_t n, int32_t D, int32_t A, int32_t t,
                                                  int32_t episode_len, int32_t slot, int32_t T, float* obs_roll,
                                                  float* act_roll, float* rew_roll, float* done_roll,
                                                  const struct smx_episode_monitor* mon, int32_t task,
                                                  const struct smx_reset_stream* resets, smx_stream_t stream) {
    return synth_task_env_step(state, init_state, actions, n, D, A, t, episode_len, slot, T, obs_roll, act_roll, rew_roll,
                               done_roll, mon, task, resets && resets->enabled ? resets : nullptr, stream);
}

extern "C" int smx_reset_fill_f32(const struct smx_reset_stream* resets, int32_t task, int32_t n, int32_t D, float* out,
                                  smx_stream_t stream) {
    const bool arm = task == SMX_TASK_ARM;           // (a task with a reset distribution and a row of D elements)
    SMX_REQUIRE(arm ? D >= 4 && D % 2 == 0 && synth_task_ok(task, D, (D - 2) / 2)
                    : task == SMX_TASK_REACH && D % 3 == 0 && synth_task_ok(task, D, D / 3), SMX_E_UNSUPPORTED);
    SMX_REQUIRE(resets && out, SMX_E_NULL);
    smx_reset_stream R = *resets;
    R.enabled = 1;
    SMX_REQUIRE(n > 0 && reset_shape_ok(R, n), SMX_E_SHAPE);
    const long total = (long)n * D;
    hipLaunchKernelGGL(arm ? arm_reset_fill_kernel : reset_fill_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       smx_s(stream), R, D, total, out);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}
