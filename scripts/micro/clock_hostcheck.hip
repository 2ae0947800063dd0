// Stand-alone host check of the per-actor clock entry points' argument validation (csrc/smx_actor_clock.hip and the two
// *_clocks_f32 entry points of csrc/smx_rollout.hip): argument blocks with deliberately bad values -- null tables, a
// clock outside its episode, rows past the ring -- must come back with their SMX_E_* code BEFORE anything is launched, so
// this runs on a machine without a GPU, and under the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/clock_hostcheck.hip surreal_amd/csrc/smx_actor_clock.hip surreal_amd/csrc/smx_rollout.hip \
//       -o scripts/micro/clock_hostcheck
//   scripts/micro/clock_hostcheck         # prints one line per case, exits 0 when every code is the expected one
// The device pointers are fakes that are never dereferenced; t_host / episode_len_host are real host arrays.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/surreal_amd.h"

static int failures = 0;

static void expect(const char* what, int got, int want) {
    printf("%-58s rc=%d %s\n", what, got, got == want ? "ok" : "UNEXPECTED");
    failures += got != want;
}

static float* fake() { return reinterpret_cast<float*>(4096); }
static const int32_t* fake_i32() { return reinterpret_cast<const int32_t*>(4096); }

static smx_actor_clock_rows rows_block(const std::vector<int32_t>* t, const std::vector<int32_t>* lens) {
    smx_actor_clock_rows p;
    memset(&p, 0, sizeof(p));
    p.n = 5; p.steps = 7; p.n_step = 4; p.advance = 3;
    p.t = fake_i32(); p.episode_len = fake_i32(); p.row_off = reinterpret_cast<int32_t*>(4096);
    p.t_host = t ? t->data() : nullptr;
    p.episode_len_host = lens ? lens->data() : nullptr;
    return p;
}

static smx_actor_clocks clocks(int64_t rows) {
    smx_actor_clocks c;
    c.t = fake_i32(); c.episode_len = fake_i32(); c.row_off = fake_i32(); c.rows = rows;
    return c;
}

static smx_mlp3_t net() {
    smx_mlp3_t n;
    memset(&n, 0, sizeof(n));
    n.D = 7; n.H1 = 24; n.H2 = 16; n.OUT = 3;
    n.W1 = n.b1 = n.W2 = n.b2 = n.W3 = n.b3 = fake();
    return n;
}

static smx_synth_ppo_window_rollout ppo(const smx_mlp3_t* n) {
    smx_synth_ppo_window_rollout p;
    memset(&p, 0, sizeof(p));
    smx_synth_rollout_t& q = p.base.roll;
    q.net = n; q.packed = fake(); q.log_var = fake(); q.state = fake(); q.init_state = fake();
    q.n = 8; q.steps = 10; q.t = 99; q.episode_len = 0;      // (the shared clock: ignored)
    p.n_step = 7; p.advance = 3;
    p.carry_obs = p.carry_act = p.carry_rew = p.carry_pd = fake();
    p.obs = p.obs_next = p.actions = p.rewards = p.dones = p.pds = fake();
    p.cursor = 0; p.capacity = 64;
    return p;
}

static smx_ddpg_rollout_t ddpg(const smx_mlp3_t* n) {
    smx_ddpg_rollout_t p;
    memset(&p, 0, sizeof(p));
    p.net = n; p.packed = fake();
    p.n = 8; p.D = 7; p.A = 3; p.steps = 10; p.n_step = 3; p.t = -5; p.episode_len = 0;      // (ignored)
    p.state = fake(); p.init_state = fake(); p.gpow = reinterpret_cast<const double*>(4096);
    p.carry_obs = p.carry_act = p.carry_rew = fake();
    p.obs = p.obs_next = p.actions = p.rewards = p.dones = fake();
    p.cursor = 0; p.capacity = 64;
    return p;
}

int main() {
    const std::vector<int32_t> t = {0, 1, 2, 3, 3}, lens = {1, 2, 3, 4, 4};
    const std::vector<int32_t> t_at_len = {0, 1, 3, 3, 3}, t_neg = {0, 1, -1, 3, 3}, len_zero = {1, 2, 0, 4, 4};

    expect("table: null argument block", smx_actor_clock_rows_i32(nullptr, nullptr), SMX_E_NULL);
    {
        auto p = rows_block(&t, &lens); p.t = nullptr;
        expect("table: null t", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_NULL);
        p = rows_block(&t, &lens); p.episode_len = nullptr;
        expect("table: null episode_len", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_NULL);
        p = rows_block(&t, &lens); p.row_off = nullptr;
        expect("table: null row_off", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_NULL);
        p = rows_block(&t_at_len, &lens);
        expect("table: t == episode_len", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(&t_neg, &lens);
        expect("table: t < 0", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(&t_neg, nullptr);
        expect("table: t < 0, no lengths on the host", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(&t, &len_zero);
        expect("table: episode_len 0", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(nullptr, &len_zero);
        expect("table: episode_len 0, no clocks on the host", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(&t, &lens); p.advance = 0;
        expect("table: advance 0", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(&t, &lens); p.advance = 5;
        expect("table: advance > n_step", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(&t, &lens); p.steps = 0;
        expect("table: steps 0", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
        p = rows_block(nullptr, nullptr); p.n = 1 << 16; p.steps = 1 << 15;
        expect("table: n * steps == 2^31", smx_actor_clock_rows_i32(&p, nullptr), SMX_E_SHAPE);
    }
    const smx_mlp3_t n = net();
    {
        auto p = ppo(&n);
        auto c = clocks(10);
        expect("ppo: null clocks", smx_synth_ppo_window_rollout_clocks_f32(&p, nullptr, nullptr), SMX_E_NULL);
        expect("ppo: null argument block", smx_synth_ppo_window_rollout_clocks_f32(nullptr, &c, nullptr), SMX_E_NULL);
        c = clocks(10); c.t = nullptr;
        expect("ppo: null clocks.t", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_NULL);
        c = clocks(10); c.episode_len = nullptr;
        expect("ppo: null clocks.episode_len", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_NULL);
        c = clocks(10); c.row_off = nullptr;
        expect("ppo: null clocks.row_off", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_NULL);
        c = clocks(65);
        expect("ppo: rows > capacity", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_SHAPE);
        c = clocks(-1);
        expect("ppo: rows < 0", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_SHAPE);
        c = clocks(10); p.pds = nullptr;
        expect("ppo: null pds table", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_NULL);
        p = ppo(&n); p.advance = 8;
        expect("ppo: advance > n_step", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_SHAPE);
        p = ppo(&n); p.cursor = 64;
        expect("ppo: cursor outside the ring", smx_synth_ppo_window_rollout_clocks_f32(&p, &c, nullptr), SMX_E_SHAPE);
    }
    {
        auto p = ddpg(&n);
        auto c = clocks(10);
        expect("ddpg: null clocks", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, nullptr, nullptr), SMX_E_NULL);
        expect("ddpg: null argument block", smx_synth_ddpg_rollout_clocks_f32(nullptr, nullptr, &c, nullptr), SMX_E_NULL);
        c = clocks(10); c.t = nullptr;
        expect("ddpg: null clocks.t", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_NULL);
        c = clocks(10); c.episode_len = nullptr;
        expect("ddpg: null clocks.episode_len", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_NULL);
        c = clocks(10); c.row_off = nullptr;
        expect("ddpg: null clocks.row_off", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_NULL);
        c = clocks(65);
        expect("ddpg: rows > capacity", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_SHAPE);
        c = clocks(10); p.obs_next = nullptr;
        expect("ddpg: null obs_next table", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_NULL);
        p = ddpg(&n); p.n_step = 0;
        expect("ddpg: n_step 0", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_SHAPE);
        p = ddpg(&n); p.actors_per_workgroup = 5;
        expect("ddpg: actors_per_workgroup 5", smx_synth_ddpg_rollout_clocks_f32(&p, nullptr, &c, nullptr), SMX_E_SHAPE);
    }
    printf("%d unexpected\n", failures);
    return failures != 0;
}
