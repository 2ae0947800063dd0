// Stand-alone host check of the argument validation of the multi-set evaluation (smx_synth_ppo_eval_sets_f32,
// smx_synth_ddpg_eval_sets_f32, smx_eval_snapshot_store_f32 and smx_eval_snapshot_floats of csrc/smx_rollout.hip): every
// refused argument block must give its code BEFORE anything is launched, so this runs on a machine without a GPU, and
// under the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/eval_sets_hostcheck.hip surreal_amd/csrc/smx_rollout.hip surreal_amd/csrc/smx_epoch.hip \
//       surreal_amd/csrc/smx_param_noise.hip -o scripts/micro/eval_sets_hostcheck
//   (smx_epoch.hip: the store packs through smx_epoch_pack_f32; smx_param_noise.hip: the size of a population's copy)
//   scripts/micro/eval_sets_hostcheck     # prints one line per case, exits 0 when every code is the expected one
// The device pointers are fakes that are never dereferenced.
#include <stdio.h>
#include <string.h>
#include "../../include/surreal_amd.h"

static int failures = 0;

static void expect(const char* what, long long got, long long want) {
    printf("%-62s rc=%lld %s\n", what, got, got == want ? "ok" : "UNEXPECTED");
    failures += got != want;
}

static float* fake(long off = 0) { return reinterpret_cast<float*>(4096 + off); }

static smx_mlp3_t net(int D, int A, int H1 = 32) {
    smx_mlp3_t n;
    memset(&n, 0, sizeof(n));
    n.D = D; n.H1 = H1; n.H2 = 32; n.OUT = A;
    n.W1 = n.b1 = n.W2 = n.b2 = n.W3 = n.b3 = fake();
    return n;
}

static smx_lstm_t lstm(int D, int H) {
    smx_lstm_t l;
    memset(&l, 0, sizeof(l));
    l.D = D; l.H = H;
    l.W_ih = l.W_hh = l.b_ih = l.b_hh = fake();
    return l;
}

// (the parameter pointers of the blocks stay NULL: the multi-set launches do not read them)
static smx_synth_ppo_eval ppo(const smx_mlp3_t* n, int task = SMX_TASK_REACH) {
    smx_synth_ppo_eval p;
    memset(&p, 0, sizeof(p));
    p.net = n; p.init_state = fake();
    p.returns = reinterpret_cast<double*>(4096);
    p.out_act = 2; p.n = 4; p.episodes = 2; p.episode_len = 3; p.task = task;
    return p;
}

static smx_synth_ddpg_eval ddpg(const smx_mlp3_t* n, int task = SMX_TASK_REACH) {
    smx_synth_ddpg_eval p;
    memset(&p, 0, sizeof(p));
    p.net = n; p.init_state = fake();
    p.returns = reinterpret_cast<double*>(4096);
    p.n = 4; p.episodes = 2; p.episode_len = 3; p.task = task;
    return p;
}

static smx_eval_sets sets_of(long long stride, int sets = 2, int zfilter = 0) {
    smx_eval_sets s;
    memset(&s, 0, sizeof(s));
    s.blobs = fake(); s.stride = stride; s.sets = sets; s.zfilter = zfilter;
    return s;
}

static smx_reset_stream rst(long long base, long long episode) {
    smx_reset_stream r;
    memset(&r, 0, sizeof(r));
    r.seed = 0x9E3779B97F4A7C15ull; r.actor_base = base; r.episode = episode; r.enabled = 1;
    return r;
}

// the checks both entry points share (make: a block maker, call: the entry point, is_ddpg: the snapshot's kind)
template <typename Make, typename Call>
static void common(const char* who, int is_ddpg, Make make, Call call) {
    char what[112];
    auto say = [&](const char* s) { snprintf(what, sizeof(what), "%s: %s", who, s); return what; };
    const smx_mlp3_t good = net(6, 2), wide = net(17, 6), odd = net(7, 2), h30 = net(6, 2, 30);
    const long long need = smx_eval_snapshot_floats(is_ddpg, 6, 0, 32, 32, 2, 0);
    auto p = make(&good, SMX_TASK_REACH);
    auto s = sets_of(need);
    expect(say("null sets"), call(&p, nullptr), SMX_E_NULL);
    s.blobs = nullptr;
    expect(say("null blobs"), call(&p, &s), SMX_E_NULL);
    s = sets_of(need, 0);
    expect(say("sets 0"), call(&p, &s), SMX_E_SHAPE);
    s = sets_of(need, 65536);
    expect(say("sets 65536"), call(&p, &s), SMX_E_SHAPE);
    s = sets_of(need, 64); p.n = 1 << 15; p.episodes = 1 << 10;
    expect(say("sets * n * episodes = 2^31"), call(&p, &s), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH);
    s = sets_of(need - 64);
    expect(say("stride below a snapshot"), call(&p, &s), SMX_E_SHAPE);
    s = sets_of(need + 2);
    expect(say("stride no multiple of 4"), call(&p, &s), SMX_E_SHAPE);
    s = sets_of(need); s.blobs = fake(8);
    expect(say("blobs on 8 bytes"), call(&p, &s), SMX_E_ALIGN);
    s = sets_of(need, 2, 2);
    expect(say("zfilter 2"), call(&p, &s), SMX_E_SHAPE);
    // what the single-set entry points refuse
    s = sets_of(need);
    p = make(&wide, SMX_TASK_DRIFT); p.resets = rst(0, 0);
    expect(say("drift with an enabled stream"), call(&p, &s), SMX_E_UNSUPPORTED);
    p = make(&odd, SMX_TASK_REACH);
    expect(say("reach, D != 3 A"), call(&p, &s), SMX_E_UNSUPPORTED);
    p = make(&good, 7);
    expect(say("unknown task"), call(&p, &s), SMX_E_UNSUPPORTED);
    p = make(&h30, SMX_TASK_REACH);
    expect(say("H1 = 30"), call(&p, &s), SMX_E_UNSUPPORTED);
    p = make(&good, SMX_TASK_REACH); p.resets = rst(-1, 0);
    expect(say("actor_base -1"), call(&p, &s), SMX_E_SHAPE);
    p.resets = rst(0, -1);
    expect(say("first_episode -1"), call(&p, &s), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.episodes = 0;
    expect(say("episodes 0"), call(&p, &s), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.n = 0;
    expect(say("n 0"), call(&p, &s), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.actors_per_workgroup = 5;
    expect(say("actors_per_workgroup 5"), call(&p, &s), SMX_E_SHAPE);
    p = make(&good, SMX_TASK_REACH); p.net = nullptr;
    expect(say("null net"), call(&p, &s), SMX_E_NULL);
    p = make(&good, SMX_TASK_REACH); p.init_state = nullptr;
    expect(say("null init_state"), call(&p, &s), SMX_E_NULL);
    p = make(&good, SMX_TASK_REACH); p.returns = nullptr;
    expect(say("null returns"), call(&p, &s), SMX_E_NULL);
    expect(say("null argument block"), call(nullptr, &s), SMX_E_NULL);
}

int main() {
    common("ppo sets", 0, [](const smx_mlp3_t* n, int task) { return ppo(n, task); },
           [](const smx_synth_ppo_eval* p, const smx_eval_sets* s) { return smx_synth_ppo_eval_sets_f32(p, s, nullptr); });
    common("ddpg sets", 1, [](const smx_mlp3_t* n, int task) { return ddpg(n, task); },
           [](const smx_synth_ddpg_eval* p, const smx_eval_sets* s) { return smx_synth_ddpg_eval_sets_f32(p, s, nullptr); });
    const smx_mlp3_t good = net(6, 2), wide = net(63, 21), stem = net(12, 2), h30 = net(6, 2, 30);
    const long long need = smx_eval_snapshot_floats(0, 6, 0, 32, 32, 2, 0);
    const long long need63 = smx_eval_snapshot_floats(0, 63, 0, 32, 32, 21, 0);
    // the z-filter's sums and the LSTM's block are part of the stride the caller sized
    auto p = ppo(&wide);
    auto s = sets_of(need63, 2, 1);
    expect("ppo sets: zfilter on a layout sized without it", smx_synth_ppo_eval_sets_f32(&p, &s, nullptr), SMX_E_SHAPE);
    auto d = ddpg(&good);
    s = sets_of(need, 2, 1);
    expect("ddpg sets: zfilter 1", smx_synth_ddpg_eval_sets_f32(&d, &s, nullptr), SMX_E_SHAPE);
    const smx_lstm_t l = lstm(6, 12);
    p = ppo(&stem); p.lstm = &l; p.hidden = 10;
    s = sets_of(need);
    expect("ppo sets: an MLP's stride under an LSTM policy", smx_synth_ppo_eval_sets_f32(&p, &s, nullptr), SMX_E_SHAPE);
    p.hidden = 5;
    expect("ppo sets: lstm padding of 7 units", smx_synth_ppo_eval_sets_f32(&p, &s, nullptr), SMX_E_SHAPE);
    p = ppo(&good); p.noise.enabled = 1; p.noise.actor_base = -1;
    expect("ppo sets: noise actor_base -1", smx_synth_ppo_eval_sets_f32(&p, &s, nullptr), SMX_E_SHAPE);

    // the store
    smx_eval_snapshot_src src;
    auto fresh = [&](const smx_mlp3_t* n, int is_ddpg) {
        memset(&src, 0, sizeof(src));
        src.net = n; src.ddpg = is_ddpg;
        if (!is_ddpg) src.log_var = fake();
    };
    expect("store: null source", smx_eval_snapshot_store_f32(nullptr, fake(), nullptr), SMX_E_NULL);
    fresh(&good, 0);
    expect("store: null blob", smx_eval_snapshot_store_f32(&src, nullptr, nullptr), SMX_E_NULL);
    src.net = nullptr;
    expect("store: null net", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_NULL);
    fresh(&good, 0); src.log_var = nullptr;
    expect("store: ppo without log_var", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_NULL);
    smx_mlp3_t holed = good;
    holed.b2 = nullptr;
    fresh(&holed, 1);
    expect("store: a net without b2", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_NULL);
    fresh(&good, 0); src.zsum = fake(); src.zsumsq = fake();
    expect("store: two of the z-filter's three", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_NULL);
    smx_lstm_t half = l;
    half.W_hh = nullptr;
    fresh(&stem, 0); src.lstm = &half;
    expect("store: an lstm without W_hh", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_NULL);
    const smx_mlp3_t stem8 = net(8, 2);
    fresh(&stem8, 0); src.lstm = &l;
    expect("store: the actor does not read the lstm's units", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_SHAPE);
    fresh(&h30, 0);
    expect("store: H1 = 30", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_UNSUPPORTED);
    fresh(&good, 1); src.zsum = src.zsumsq = src.zcount = fake();
    expect("store: a ddpg actor with a z-filter", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_UNSUPPORTED);
    fresh(&stem, 1); src.lstm = &l;
    expect("store: a ddpg actor with an lstm", smx_eval_snapshot_store_f32(&src, fake(), nullptr), SMX_E_UNSUPPORTED);
    fresh(&good, 0);
    expect("store: blob on 4 bytes", smx_eval_snapshot_store_f32(&src, fake(4), nullptr), SMX_E_ALIGN);

    // the size query
    expect("floats: ddpg = one copy of a population", smx_eval_snapshot_floats(1, 6, 0, 32, 32, 2, 0),
           smx_param_noise_copy_floats(6, 32, 32, 2, 0));
    expect("floats: ddpg ragged = one copy", smx_eval_snapshot_floats(1, 17, 0, 28, 20, 6, 0),
           smx_param_noise_copy_floats(17, 28, 20, 6, 0));
    expect("floats: a multiple of 64", smx_eval_snapshot_floats(0, 63, 12, 28, 20, 21, 1) % 64, 0);
    expect("floats: the sums make a 63-wide layout longer", smx_eval_snapshot_floats(0, 63, 0, 32, 32, 21, 1) > need63, 1);
    expect("floats: H1 = 30", smx_eval_snapshot_floats(0, 6, 0, 30, 32, 2, 0), 0);
    expect("floats: ddpg with LSTM units", smx_eval_snapshot_floats(1, 6, 12, 32, 32, 2, 0), 0);
    expect("floats: ddpg with a z-filter", smx_eval_snapshot_floats(1, 6, 0, 32, 32, 2, 1), 0);
    expect("floats: zfilter 2", smx_eval_snapshot_floats(0, 6, 0, 32, 32, 2, 2), 0);
    printf("%d unexpected\n", failures);
    return failures != 0;
}
