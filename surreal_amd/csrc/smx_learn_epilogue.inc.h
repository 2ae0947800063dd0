// What PPOLearner._optimize does after its epoch loops (ppo.py:565-584): the explained variance / value loss of every
// value epoch from their block moments, the moments of the return targets, the z-filter update on the step-0
// observations -- independent pieces, one per group of role workgroups -- and, by the last role workgroup to finish, the
// means the learner reports (they read the UPDATED z-filter sums).  Role workgroup r of `count`:
//   r < nz         column sums of 64 observation features (the z-filter update; zupdate_kernel is this role alone)
//   r == nz        moments of `ret`
//   r > nz         value-loss finalize, 16 epochs (waves) per workgroup
// ONE definition for the two launches that run them: learn_epilogue_kernel (smx_scan.hip: its own launch, 1024 threads)
// and epoch_fwd_final*_kernel (smx_epoch.hip: the workgroups behind the row blocks of the learn's final forward-only
// launch, 512 threads).  Both must write the same bits, so everything here is 1024 VIRTUAL threads on NTH real ones:
// thread t plays the virtual threads t, t + NTH, ... one after the other -- with NTH = 512, virtual wave w + 8 is real wave
// w with the same lanes -- so every per-thread chain, every wave butterfly and every fixed-order sum over the sixteen
// waves has the operands and the order it has on 1024 threads (smx_moments.inc.h); with NTH = 1024 the pass loops have
// one trip.  How a role's words reach the last role workgroup is the launch's own business (COH):
//   COH = false    a launch of its own: plain stores, a ticket between device-scope fences (last_block_done)
//   COH = true     beside workgroups whose activations are dirty in L2: the running sums and the count travel as
//                  device-scope stores and loads (no fence: see partial_store, smx_ppo_loss.inc.h), counted by a relaxed
//                  ticket over the `count` role workgroups alone
// COH selects the store of a running sum, the load of one and the "am I last" step: no loop and no sum exists twice.
// Included at file scope.
#pragma once
#include "smx_moments.inc.h"

struct EpilogueArgs {
    const float* x; long ldx; long rows; int D;
    float *rs, *rsq, *cnt; float count_rows;
    const float* ret; long n_ret; float* ret_mom;
    const float* vpartials; int n_epochs, nblk; float* vstats; int vstride;
    const float* log_var; int A; float* out4;
    int* ticket;
    int nz, count;     // column blocks of the z-update / workgroups of all roles
};

// checks a, fills P; returns the role workgroups to launch (> 0), or the SMX_E_* code
static inline int learn_epilogue_args(const smx_learn_epilogue_t* a, EpilogueArgs& P) {
    SMX_REQUIRE(a && a->ret && a->ret_moments && a->log_var && a->out4 && a->ticket, SMX_E_NULL);
    SMX_REQUIRE(a->n_ret > 0 && a->A > 0, SMX_E_SHAPE);
    SMX_REQUIRE(!a->x || (a->running_sum && a->running_sumsq && a->count && a->rows > 0 && a->D > 0 && a->ldx >= a->D),
                SMX_E_SHAPE);
    SMX_REQUIRE(a->n_epochs == 0 || (a->v_partials && a->v_stats && a->nblk > 0 && a->stats_stride >= 2), SMX_E_SHAPE);
    SMX_REQUIRE(a->n_epochs == 0 || ((uintptr_t)a->v_partials & 15) == 0, SMX_E_ALIGN);
    P.x = a->x; P.ldx = (long)a->ldx; P.rows = (long)a->rows; P.D = a->D;
    P.rs = a->running_sum; P.rsq = a->running_sumsq; P.cnt = a->count; P.count_rows = a->count_rows;
    P.ret = a->ret; P.n_ret = (long)a->n_ret; P.ret_mom = a->ret_moments;
    P.vpartials = a->v_partials; P.n_epochs = a->n_epochs; P.nblk = a->nblk; P.vstats = a->v_stats;
    P.vstride = a->stats_stride;
    P.log_var = a->log_var; P.A = a->A; P.out4 = a->out4; P.ticket = (int*)a->ticket;
    P.nz = a->x ? (a->D + 63) / 64 : 0;
    P.count = P.nz + 1 + (a->n_epochs + 15) / 16;
    return P.count;
}

// the LAST workgroup of a launch to get here returns true (device-scope release / acquire around a
// ticket counter, which it resets for the next launch): the place for a launch's global epilogue
static __device__ __forceinline__ bool last_block_done(int* ticket) {
    __shared__ int is_last;
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const int t = atomicAdd(ticket, 1);
        is_last = (t == (int)gridDim.x - 1);
        if (is_last) *ticket = 0;
        __threadfence();
    }
    __syncthreads();
    return is_last != 0;
}

// Column sums of x and x*x into the running sums, block `blk` = 64 columns x 16 row-lanes (1024 virtual threads); each
// walks rows r = g, g+16, ... (the rows of obs[:, 0, :] are N*D floats apart: latency-bound, so depth comes from 16
// row-lanes x 16 independent loads in flight), then a fixed-order LDS reduction.  s1, s2: 16 x 64 floats of LDS each.
template <int NTH, bool COH>
static __device__ __forceinline__ void zfilter_column_sums(const float* __restrict__ x, const long ldx, const long rows,
                                                           const int D, const int blk, float* rs, float* rsq, float* cnt,
                                                           const float count_rows, float* s1, float* s2) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int ps = 0; ps < 1024 / NTH; ++ps) {
        const int vt = tid + NTH * ps;
        const int c = vt & 63, g = vt >> 6;
        const int col = blk * 64 + c;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, q0 = 0.f, q1 = 0.f, q2 = 0.f, q3 = 0.f;
        if (col < D) {
            long r = g;
            // (sixteen loads in flight; the additions in the order of four passes of the loop below: bit-identical sums.
            // With four in flight a thread's 64 rows were sixteen dependent round trips -- 10 of the epilogue launch's 12 us)
            for (; r + 240 < rows; r += 256) {
                float v[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) v[i] = x[(r + 16 * i) * ldx + col];
#pragma unroll
                for (int i = 0; i < 16; i += 4) {
                    a0 += v[i]; q0 += v[i] * v[i];
                    a1 += v[i + 1]; q1 += v[i + 1] * v[i + 1];
                    a2 += v[i + 2]; q2 += v[i + 2] * v[i + 2];
                    a3 += v[i + 3]; q3 += v[i + 3] * v[i + 3];
                }
            }
            for (; r + 48 < rows; r += 64) {
                const float v0 = x[r * ldx + col], v1 = x[(r + 16) * ldx + col];
                const float v2 = x[(r + 32) * ldx + col], v3 = x[(r + 48) * ldx + col];
                a0 += v0; q0 += v0 * v0;
                a1 += v1; q1 += v1 * v1;
                a2 += v2; q2 += v2 * v2;
                a3 += v3; q3 += v3 * v3;
            }
            for (; r < rows; r += 16) {
                const float v = x[r * ldx + col];
                a0 += v; q0 += v * v;
            }
        }
        s1[g * 64 + c] = (a0 + a1) + (a2 + a3);
        s2[g * 64 + c] = (q0 + q1) + (q2 + q3);
    }
    __syncthreads();
    const int col = blk * 64 + tid;
    if (tid < 64 && col < D) {                   // (virtual row-lane 0)
        float ta = 0.f, tq = 0.f;
        for (int k = 0; k < 16; ++k) { ta += s1[k * 64 + tid]; tq += s2[k * 64 + tid]; }
        stat_store<COH>(rs + col, rs[col] + ta);      // z_filter.py:55
        stat_store<COH>(rsq + col, rsq[col] + tq);    // z_filter.py:56
    }
    if (blk == 0 && tid == 0) stat_store<COH>(cnt, cnt[0] + count_rows);   // z_filter.py:57
}

// role workgroup blk.  LDS: s1, s2 (16 x 64 floats each), red (16 x 4 doubles; the moments use the first 16), one
// broadcast double, and (COH) one int
template <int NTH, bool COH>
static __device__ __forceinline__ void learn_epilogue_roles(const EpilogueArgs& P, const int blk, float* s1, float* s2,
                                                            double (*red)[4], double* bc, int* is_last) {
    const int tid = threadIdx.x;
    if (blk < P.nz) {
        zfilter_column_sums<NTH, COH>(P.x, P.ldx, P.rows, P.D, blk, P.rs, P.rsq, P.cnt, P.count_rows, s1, s2);
    } else if (blk == P.nz) {
        block_moments<1024, NTH>(P.ret, P.n_ret, P.ret_mom, &red[0][0], bc);
    } else {
#pragma unroll
        for (int ps = 0; ps < 1024 / NTH; ++ps) {
            const int e = (blk - P.nz - 1) * 16 + ((tid + NTH * ps) >> 6);
            if (e < P.n_epochs)
                value_finalize_wave(P.vpartials + (size_t)e * P.nblk * 8, P.nblk, P.vstats + (size_t)e * P.vstride,
                                    tid & 63);
        }
    }
    if constexpr (COH) {
        // the last role workgroup to get here (its ticket counts them alone: they run whether or not the policy has stopped)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            const int t = __hip_atomic_fetch_add(P.ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = t == P.count - 1;
            if (last) __hip_atomic_store(P.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *is_last = last;
        }
        __syncthreads();
        if (*is_last == 0) return;
    } else {
        if (!last_block_done(P.ticket)) return;
    }
    final_stats_block<1024, NTH, COH>(P.log_var, P.A, P.nz ? P.rs : nullptr, P.rsq, P.cnt, P.D, P.out4, red);
}
