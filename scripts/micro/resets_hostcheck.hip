// Stand-alone host check of the reset-stream entry points' argument validation (smx_reset_fill_f32 and the three
// smx_synth_*_resets_f32 entry points of csrc/smx_rollout.hip and csrc/smx_replay.hip): a NULL stream and a disabled one
// must give the task entry point's code, an enabled stream on SMX_TASK_DRIFT SMX_E_UNSUPPORTED, a global actor id outside
// [0, 2^32) or a negative episode SMX_E_SHAPE -- all BEFORE anything is launched, so this runs on a machine without a
// GPU, and under the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/resets_hostcheck.hip surreal_amd/csrc/smx_rollout.hip surreal_amd/csrc/smx_replay.hip \
//       -o scripts/micro/resets_hostcheck
//   scripts/micro/resets_hostcheck        # prints one line per case, exits 0 when every code is the expected one
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

static smx_reset_stream rst(long long base, long long episode, int enabled = 1) {
    smx_reset_stream r;
    memset(&r, 0, sizeof(r));
    r.seed = 0x9E3779B97F4A7C15ull; r.actor_base = base; r.episode = episode; r.enabled = enabled;
    return r;
}

static int step(int task, const smx_reset_stream* r, float* state = fake(), int D = 6, int A = 2) {
    return smx_synth_task_env_step_resets_f32(state, fake(), fake(), 8, D, A, 0, 5, 0, 1, nullptr, nullptr, nullptr,
                                              nullptr, nullptr, task, r, nullptr);
}

int main() {
    const long long top = 1LL << 32;
    const smx_reset_stream ok = rst(0, 0), off = rst(-1, -1, 0), low = rst(-1, 0), high = rst(top - 7, 0), neg = rst(0, -1);
    const smx_reset_stream edge = rst(top - 8, 0x7FFFFFFFFFFFFFFFll);

    expect("fill: drift", smx_reset_fill_f32(&ok, SMX_TASK_DRIFT, 8, 6, fake(), nullptr), SMX_E_UNSUPPORTED);
    expect("fill: unknown task", smx_reset_fill_f32(&ok, 7, 8, 6, fake(), nullptr), SMX_E_UNSUPPORTED);
    expect("fill: D = 7", smx_reset_fill_f32(&ok, SMX_TASK_REACH, 8, 7, fake(), nullptr), SMX_E_UNSUPPORTED);
    expect("fill: D = 66", smx_reset_fill_f32(&ok, SMX_TASK_REACH, 8, 66, fake(), nullptr), SMX_E_UNSUPPORTED);
    expect("fill: null stream", smx_reset_fill_f32(nullptr, SMX_TASK_REACH, 8, 6, fake(), nullptr), SMX_E_NULL);
    expect("fill: null out", smx_reset_fill_f32(&ok, SMX_TASK_REACH, 8, 6, nullptr, nullptr), SMX_E_NULL);
    expect("fill: n = 0", smx_reset_fill_f32(&ok, SMX_TASK_REACH, 0, 6, fake(), nullptr), SMX_E_SHAPE);
    expect("fill: actor_base -1", smx_reset_fill_f32(&low, SMX_TASK_REACH, 8, 6, fake(), nullptr), SMX_E_SHAPE);
    expect("fill: actor_base + n > 2^32", smx_reset_fill_f32(&high, SMX_TASK_REACH, 8, 6, fake(), nullptr), SMX_E_SHAPE);
    expect("fill: episode -1", smx_reset_fill_f32(&neg, SMX_TASK_REACH, 8, 6, fake(), nullptr), SMX_E_SHAPE);
    expect("fill: a disabled stream's base is still checked", smx_reset_fill_f32(&off, SMX_TASK_REACH, 8, 6, fake(), nullptr),
           SMX_E_SHAPE);

    expect("step: drift with a stream", step(SMX_TASK_DRIFT, &ok), SMX_E_UNSUPPORTED);
    expect("step: unknown task with a stream", step(7, &ok), SMX_E_UNSUPPORTED);
    expect("step: actor_base -1", step(SMX_TASK_REACH, &low), SMX_E_SHAPE);
    expect("step: actor_base + n > 2^32", step(SMX_TASK_REACH, &high), SMX_E_SHAPE);
    expect("step: episode -1", step(SMX_TASK_REACH, &neg), SMX_E_SHAPE);
    expect("step: null state (the task entry point's check)", step(SMX_TASK_REACH, &edge, nullptr), SMX_E_NULL);
    expect("step: D != 3 A (the task entry point's check)", step(SMX_TASK_REACH, &ok, fake(), 7, 2), SMX_E_UNSUPPORTED);
    expect("step: null stream, null state", step(SMX_TASK_REACH, nullptr, nullptr), SMX_E_NULL);
    expect("step: disabled stream, null state", step(SMX_TASK_REACH, &off, nullptr), SMX_E_NULL);
    expect("step: disabled stream, drift forwards, null state", step(SMX_TASK_DRIFT, &off, nullptr, 7, 2), SMX_E_NULL);
    expect("step: null stream, drift forwards, null state", step(SMX_TASK_DRIFT, nullptr, nullptr, 7, 2), SMX_E_NULL);

    const smx_mlp3_t good = net(6, 2), odd = net(7, 2);
    {
        auto p = ppo(&good);
        expect("ppo: drift with a stream", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_DRIFT, &ok, nullptr), SMX_E_UNSUPPORTED);
        expect("ppo: unknown task with a stream", smx_synth_ppo_window_rollout_resets_f32(&p, 7, &ok, nullptr), SMX_E_UNSUPPORTED);
        expect("ppo: actor_base -1", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_REACH, &low, nullptr), SMX_E_SHAPE);
        expect("ppo: actor_base + n > 2^32", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_REACH, &high, nullptr), SMX_E_SHAPE);
        expect("ppo: episode -1", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_REACH, &neg, nullptr), SMX_E_SHAPE);
        expect("ppo: null argument block", smx_synth_ppo_window_rollout_resets_f32(nullptr, SMX_TASK_REACH, &ok, nullptr), SMX_E_NULL);
        expect("ppo: null stream, null argument block", smx_synth_ppo_window_rollout_resets_f32(nullptr, SMX_TASK_REACH, nullptr, nullptr),
               SMX_E_NULL);
        expect("ppo: disabled stream, drift forwards, null block", smx_synth_ppo_window_rollout_resets_f32(nullptr, SMX_TASK_DRIFT, &off, nullptr),
               SMX_E_NULL);
        p = ppo(&good); p.pds = nullptr;
        expect("ppo: disabled stream, null pds table", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_REACH, &off, nullptr), SMX_E_NULL);
        expect("ppo: enabled stream, null pds table", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_REACH, &edge, nullptr), SMX_E_NULL);
        p = ppo(&odd);
        expect("ppo: D != 3 A", smx_synth_ppo_window_rollout_resets_f32(&p, SMX_TASK_REACH, &ok, nullptr), SMX_E_UNSUPPORTED);
    }
    {
        auto p = ddpg(&good);
        expect("ddpg: drift with a stream", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_DRIFT, &ok, nullptr), SMX_E_UNSUPPORTED);
        expect("ddpg: unknown task with a stream", smx_synth_ddpg_rollout_resets_f32(&p, 7, &ok, nullptr), SMX_E_UNSUPPORTED);
        expect("ddpg: actor_base -1", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_REACH, &low, nullptr), SMX_E_SHAPE);
        expect("ddpg: actor_base + n > 2^32", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_REACH, &high, nullptr), SMX_E_SHAPE);
        expect("ddpg: episode -1", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_REACH, &neg, nullptr), SMX_E_SHAPE);
        expect("ddpg: null argument block", smx_synth_ddpg_rollout_resets_f32(nullptr, SMX_TASK_REACH, &ok, nullptr), SMX_E_NULL);
        expect("ddpg: null stream, null argument block", smx_synth_ddpg_rollout_resets_f32(nullptr, SMX_TASK_REACH, nullptr, nullptr),
               SMX_E_NULL);
        expect("ddpg: disabled stream, drift forwards, null block", smx_synth_ddpg_rollout_resets_f32(nullptr, SMX_TASK_DRIFT, &off, nullptr),
               SMX_E_NULL);
        p = ddpg(&good); p.obs_next = nullptr;
        expect("ddpg: disabled stream, null obs_next table", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_REACH, &off, nullptr), SMX_E_NULL);
        expect("ddpg: enabled stream, null obs_next table", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_REACH, &edge, nullptr), SMX_E_NULL);
        p = ddpg(&odd);
        expect("ddpg: D != 3 A", smx_synth_ddpg_rollout_resets_f32(&p, SMX_TASK_REACH, &ok, nullptr), SMX_E_UNSUPPORTED);
    }
    printf("%d unexpected\n", failures);
    return failures != 0;
}
