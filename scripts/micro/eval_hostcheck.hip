// Stand-alone host check of the evaluation entry points' argument validation (smx_synth_ppo_eval_f32,
// smx_synth_ddpg_eval_f32 and smx_synth_eval_supported of csrc/smx_rollout.hip): an enabled reset stream on SMX_TASK_DRIFT
// and what smx_synth_task_supported or the shape query refuses must give SMX_E_UNSUPPORTED, ids outside [0, 2^32), a
// negative episode and sizes out of range SMX_E_SHAPE, a missing pointer SMX_E_NULL -- all BEFORE anything is launched, so
// this runs on a machine without a GPU, and under the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/eval_hostcheck.hip surreal_amd/csrc/smx_rollout.hip -o scripts/micro/eval_hostcheck
//   scripts/micro/eval_hostcheck          # prints one line per case, exits 0 when every code is the expected one
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

static smx_mlp3_t net(int D, int A, int H1 = 32) {
    smx_mlp3_t n;
    memset(&n, 0, sizeof(n));
    n.D = D; n.H1 = H1; n.H2 = 32; n.OUT = A;
    n.W1 = n.b1 = n.W2 = n.b2 = n.W3 = n.b3 = fake();
    return n;
}

static smx_synth_ppo_eval ppo(const smx_mlp3_t* n, int task = SMX_TASK_REACH) {
    smx_synth_ppo_eval p;
    memset(&p, 0, sizeof(p));
    p.net = n; p.packed = fake(); p.log_var = fake(); p.init_state = fake();
    p.returns = reinterpret_cast<double*>(4096);
    p.out_act = 2; p.n = 4; p.episodes = 2; p.episode_len = 3; p.task = task;
    return p;
}

static smx_synth_ddpg_eval ddpg(const smx_mlp3_t* n, int task = SMX_TASK_REACH) {
    smx_synth_ddpg_eval p;
    memset(&p, 0, sizeof(p));
    p.net = n; p.packed = fake(); p.init_state = fake();
    p.returns = reinterpret_cast<double*>(4096);
    p.n = 4; p.episodes = 2; p.episode_len = 3; p.task = task;
    return p;
}

static smx_reset_stream rst(long long base, long long episode, int enabled = 1) {
    smx_reset_stream r;
    memset(&r, 0, sizeof(r));
    r.seed = 0x9E3779B97F4A7C15ull; r.actor_base = base; r.episode = episode; r.enabled = enabled;
    return r;
}

// the checks both argument blocks share (P: a block maker, F: the entry point)
template <typename Make, typename Call>
static void common(const char* who, Make make, Call call) {
    char what[96];
    auto say = [&](const char* s) { snprintf(what, sizeof(what), "%s: %s", who, s); return what; };
    const long long top = 1LL << 32;
    const smx_mlp3_t good = net(6, 2), wide = net(17, 6), odd = net(7, 2), big = net(66, 22), h30 = net(6, 2, 30);
    auto p = make(&wide, SMX_TASK_DRIFT);
    p.resets = rst(0, 0);
    expect(say("drift with an enabled stream"), call(&p), SMX_E_UNSUPPORTED);
    p = make(&odd, SMX_TASK_REACH);
    expect(say("reach, D != 3 A"), call(&p), SMX_E_UNSUPPORTED);
    p = make(&big, SMX_TASK_REACH);
    expect(say("reach, A = 22"), call(&p), SMX_E_UNSUPPORTED);
    p = make(&good, 7);
    expect(say("unknown task"), call(&p), SMX_E_UNSUPPORTED);
    p = make(&h30, SMX_TASK_REACH);
    expect(say("H1 = 30"), call(&p), SMX_E_UNSUPPORTED);
    p = make(&good, SMX_TASK_REACH); p.resets = rst(-1, 0);
    expect(say("actor_base -1"), call(&p), SMX_E_SHAPE);
    p.resets = rst(top - 3, 0);
    expect(say("actor_base + n > 2^32"), call(&p), SMX_E_SHAPE);
    p.resets = rst(0, -1);
    expect(say("first_episode -1"), call(&p), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.episodes = 0;
    expect(say("episodes 0"), call(&p), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.episode_len = 0;
    expect(say("episode_len 0"), call(&p), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.n = 0;
    expect(say("n 0"), call(&p), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.n = 1 << 20; p.episodes = 1 << 11;
    expect(say("n * episodes = 2^31"), call(&p), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.actors_per_workgroup = 5;
    expect(say("actors_per_workgroup 5"), call(&p), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.net = nullptr;
    expect(say("null net"), call(&p), SMX_E_NULL);
    p = make(&good, SMX_TASK_REACH); p.packed = nullptr;
    expect(say("null packed"), call(&p), SMX_E_NULL);
    p = make(&good, SMX_TASK_REACH); p.init_state = nullptr;
    expect(say("null init_state"), call(&p), SMX_E_NULL);
    p = make(&good, SMX_TASK_REACH); p.returns = nullptr;
    expect(say("null returns"), call(&p), SMX_E_NULL);
    p = make(&wide, SMX_TASK_DRIFT); p.resets = rst(-1, -1, 0); p.returns = nullptr;
    expect(say("a disabled stream is not looked at"), call(&p), SMX_E_NULL);
}

int main() {
    common("ppo", [](const smx_mlp3_t* n, int task) { return ppo(n, task); },
           [](const smx_synth_ppo_eval* p) { return smx_synth_ppo_eval_f32(p, nullptr); });
    common("ddpg", [](const smx_mlp3_t* n, int task) { return ddpg(n, task); },
           [](const smx_synth_ddpg_eval* p) { return smx_synth_ddpg_eval_f32(p, nullptr); });
    expect("ppo: null argument block", smx_synth_ppo_eval_f32(nullptr, nullptr), SMX_E_NULL);
    expect("ddpg: null argument block", smx_synth_ddpg_eval_f32(nullptr, nullptr), SMX_E_NULL);
    const smx_mlp3_t good = net(6, 2);
    auto p = ppo(&good);
    p.log_var = nullptr;
    expect("ppo: null log_var", smx_synth_ppo_eval_f32(&p, nullptr), SMX_E_NULL);
    p = ppo(&good); p.zsum = fake();
    expect("ppo: one of the z-filter's three", smx_synth_ppo_eval_f32(&p, nullptr), SMX_E_NULL);
    p = ppo(&good); p.noise.enabled = 1; p.noise.actor_base = -1;
    expect("ppo: noise actor_base -1", smx_synth_ppo_eval_f32(&p, nullptr), SMX_E_SHAPE);
    smx_lstm_t l;
    memset(&l, 0, sizeof(l));
    l.D = 6; l.H = 12;
    const smx_mlp3_t stem = net(12, 2);
    p = ppo(&stem); p.lstm = &l; p.hidden = 10;
    expect("ppo: lstm without its packed weights", smx_synth_ppo_eval_f32(&p, nullptr), SMX_E_NULL);
    p.lstm_packed = fake(); p.hidden = 5;
    expect("ppo: lstm padding of 7 units", smx_synth_ppo_eval_f32(&p, nullptr), SMX_E_SHAPE);
    p.hidden = 10; p.episodes = 0;
    expect("ppo: lstm, episodes 0", smx_synth_ppo_eval_f32(&p, nullptr), SMX_E_SHAPE);
    expect("supported: ppo mlp reach", smx_synth_eval_supported(0, SMX_TASK_REACH, 6, 0, 32, 32, 2), 1);
    expect("supported: ppo lstm reach", smx_synth_eval_supported(0, SMX_TASK_REACH, 6, 12, 32, 32, 2), 1);
    expect("supported: ddpg drift ragged", smx_synth_eval_supported(1, SMX_TASK_DRIFT, 17, 0, 28, 20, 6), 1);
    expect("supported: ddpg with LSTM units", smx_synth_eval_supported(1, SMX_TASK_REACH, 6, 12, 32, 32, 2), 0);
    expect("supported: H = 10", smx_synth_eval_supported(0, SMX_TASK_REACH, 6, 10, 32, 32, 2), 0);
    expect("supported: A = 33", smx_synth_eval_supported(0, SMX_TASK_DRIFT, 17, 0, 32, 32, 33), 0);
    printf("%d unexpected\n", failures);
    return failures != 0;
}
