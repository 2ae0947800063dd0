// Stand-alone host check of the task entry points' argument validation (smx_synth_task_supported and the three
// smx_synth_*_task_f32 entry points of csrc/smx_rollout.hip and csrc/smx_replay.hip): an unknown task, D != 3 A, A > 21
// and the forwarded entry points' own null / shape checks must come back with their SMX_E_* code BEFORE anything is
// launched, so this runs on a machine without a GPU, and under the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/task_hostcheck.hip surreal_amd/csrc/smx_rollout.hip surreal_amd/csrc/smx_replay.hip \
//       -o scripts/micro/task_hostcheck
//   scripts/micro/task_hostcheck          # prints one line per case, exits 0 when every code is the expected one
// The device pointers are fakes that are never dereferenced.
#include <stdio.h>
#include <string.h>
#include "../../include/surreal_amd.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    printf("%-58s rc=%d %s\n", what, got, got == want ? "ok" : "UNEXPECTED");
    failures += got != want;
}

static float* fake() { return reinterpret_cast<float*>(4096); }

static smx_mlp3_t net(int D, int A) {
    smx_mlp3_t n;
    memset(&n, 0, sizeof(n));
    n.D = D; n.H1 = 8; n.H2 = 4; n.OUT = A;
    n.W1 = n.b1 = n.W2 = n.b2 = n.W3 = n.b3 = fake();
    return n;
}

static smx_synth_ppo_window_rollout ppo(const smx_mlp3_t* n) {
    smx_synth_ppo_window_rollout p;
    memset(&p, 0, sizeof(p));
    smx_synth_rollout_t& q = p.base.roll;
    q.net = n; q.packed = fake(); q.log_var = fake(); q.state = fake(); q.init_state = fake();
    q.n = 8; q.steps = 10; q.t = 0; q.episode_len = 5;
    p.n_step = 3; p.advance = 2;
    p.carry_obs = p.carry_act = p.carry_rew = p.carry_pd = fake();
    p.obs = p.obs_next = p.actions = p.rewards = p.dones = p.pds = fake();
    p.cursor = 0; p.capacity = 64;
    return p;
}

static smx_ddpg_rollout_t ddpg(const smx_mlp3_t* n) {
    smx_ddpg_rollout_t p;
    memset(&p, 0, sizeof(p));
    p.net = n; p.packed = fake();
    p.n = 8; p.D = n->D; p.A = n->OUT; p.steps = 4; p.n_step = 3; p.t = 0; p.episode_len = 5;
    p.state = fake(); p.init_state = fake(); p.gpow = reinterpret_cast<const double*>(4096);
    p.carry_obs = p.carry_act = p.carry_rew = fake();
    p.obs = p.obs_next = p.actions = p.rewards = p.dones = fake();
    p.cursor = 0; p.capacity = 64;
    return p;
}

static int step(int D, int A, int task, float* state = fake(), int T = 1) {
    return smx_synth_task_env_step_f32(state, fake(), fake(), 4, D, A, 0, 5, 0, T, nullptr, nullptr, nullptr, nullptr,
                                       nullptr, task, nullptr);
}

int main() {
    expect("supported: reach 3 / 1", smx_synth_task_supported(SMX_TASK_REACH, 3, 1), 1);
    expect("supported: reach 63 / 21", smx_synth_task_supported(SMX_TASK_REACH, 63, 21), 1);
    expect("supported: reach 66 / 22", smx_synth_task_supported(SMX_TASK_REACH, 66, 22), 0);
    expect("supported: reach 7 / 2", smx_synth_task_supported(SMX_TASK_REACH, 7, 2), 0);
    expect("supported: reach 0 / 0", smx_synth_task_supported(SMX_TASK_REACH, 0, 0), 0);
    expect("supported: drift 376 / 17", smx_synth_task_supported(SMX_TASK_DRIFT, 376, 17), 1);
    expect("supported: task 7", smx_synth_task_supported(7, 3, 1), 0);
    expect("supported: task -1", smx_synth_task_supported(-1, 3, 1), 0);

    expect("step: unknown task", step(6, 2, 7), SMX_E_UNSUPPORTED);
    expect("step: D != 3 A", step(7, 2, SMX_TASK_REACH), SMX_E_UNSUPPORTED);
    expect("step: A = 22", step(66, 22, SMX_TASK_REACH), SMX_E_UNSUPPORTED);
    expect("step: null state", step(6, 2, SMX_TASK_REACH, nullptr), SMX_E_NULL);
    expect("step: T = 0", step(6, 2, SMX_TASK_REACH, fake(), 0), SMX_E_SHAPE);
    expect("step: drift forwards, null state", step(7, 2, SMX_TASK_DRIFT, nullptr), SMX_E_NULL);

    const smx_mlp3_t ok = net(6, 2), odd = net(7, 2), wide = net(66, 22);
    {
        auto p = ppo(&ok);
        expect("ppo: unknown task", smx_synth_ppo_window_rollout_task_f32(&p, 7, nullptr), SMX_E_UNSUPPORTED);
        expect("ppo: null argument block", smx_synth_ppo_window_rollout_task_f32(nullptr, SMX_TASK_REACH, nullptr), SMX_E_NULL);
        expect("ppo: drift forwards, null argument block", smx_synth_ppo_window_rollout_task_f32(nullptr, SMX_TASK_DRIFT, nullptr),
               SMX_E_NULL);
        p = ppo(&odd);
        expect("ppo: D != 3 A", smx_synth_ppo_window_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_UNSUPPORTED);
        p = ppo(&wide);
        expect("ppo: A = 22", smx_synth_ppo_window_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_UNSUPPORTED);
        p = ppo(&ok); p.pds = nullptr;
        expect("ppo: null pds table", smx_synth_ppo_window_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_NULL);
        p = ppo(&ok); p.advance = 4;
        expect("ppo: advance > n_step", smx_synth_ppo_window_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_SHAPE);
        p = ppo(&ok); p.base.roll.actors_per_workgroup = 5;
        expect("ppo: actors_per_workgroup 5", smx_synth_ppo_window_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_SHAPE);
    }
    {
        auto p = ddpg(&ok);
        expect("ddpg: unknown task", smx_synth_ddpg_rollout_task_f32(&p, 7, nullptr), SMX_E_UNSUPPORTED);
        expect("ddpg: null argument block", smx_synth_ddpg_rollout_task_f32(nullptr, SMX_TASK_REACH, nullptr), SMX_E_NULL);
        expect("ddpg: drift forwards, null argument block", smx_synth_ddpg_rollout_task_f32(nullptr, SMX_TASK_DRIFT, nullptr),
               SMX_E_NULL);
        p = ddpg(&odd);
        expect("ddpg: D != 3 A", smx_synth_ddpg_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_UNSUPPORTED);
        p = ddpg(&wide);
        expect("ddpg: A = 22", smx_synth_ddpg_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_UNSUPPORTED);
        p = ddpg(&ok); p.obs_next = nullptr;
        expect("ddpg: null obs_next table", smx_synth_ddpg_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_NULL);
        p = ddpg(&ok); p.n_step = 0;
        expect("ddpg: n_step 0", smx_synth_ddpg_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_SHAPE);
        p = ddpg(&ok); p.capacity = 8;
        expect("ddpg: rows > capacity", smx_synth_ddpg_rollout_task_f32(&p, SMX_TASK_REACH, nullptr), SMX_E_SHAPE);
    }
    printf("%d unexpected\n", failures);
    return failures != 0;
}
