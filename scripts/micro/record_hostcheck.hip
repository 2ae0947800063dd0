// Stand-alone host check of the record entry points' argument validation (csrc/smx_record.hip): argument blocks with
// deliberately bad values -- null tables, rank >= n, n > capacity, a negative clock -- must come back with their SMX_E_*
// code BEFORE anything is launched, so this runs on a machine without a GPU, and under the host sanitizers:
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/record_hostcheck.hip surreal_amd/csrc/smx_record.hip -o scripts/micro/record_hostcheck
//   scripts/micro/record_hostcheck        # prints one line per case, exits 0 when every code is the expected one
// The device pointers are fakes that are never dereferenced; t_host / rank_host are real host arrays.
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

template <typename Block>
static void fill_shared(Block& p, const std::vector<int32_t>& t, const std::vector<int32_t>& rank) {
    memset(&p, 0, sizeof(p));
    p.n = (int32_t)t.size(); p.D = 7; p.A = 3; p.n_step = 4; p.rows = 2;
    p.t = p.rank = reinterpret_cast<const int32_t*>(4096);
    p.t_host = t.data(); p.rank_host = rank.data();
    p.cur_obs = fake(); p.step_actions = fake(); p.step_obs_next = fake(); p.step_rewards = fake();
    p.step_dones = fake(); p.step_obs_reset = fake();
    p.carry_obs = fake(); p.carry_act = fake(); p.carry_rew = fake();
    p.obs = fake(); p.obs_next = fake(); p.actions = fake(); p.rewards = fake(); p.dones = fake();
    p.cursor = 0; p.capacity = 64;
}

static smx_record_ppo_window_step ppo(const std::vector<int32_t>& t, const std::vector<int32_t>& rank) {
    smx_record_ppo_window_step p;
    fill_shared(p, t, rank);
    p.advance = 3; p.step_pds = fake(); p.carry_pd = fake(); p.pds = fake();
    return p;
}

static smx_record_ddpg_nstep_step ddpg(const std::vector<int32_t>& t, const std::vector<int32_t>& rank) {
    smx_record_ddpg_nstep_step p;
    fill_shared(p, t, rank);
    p.gpow = reinterpret_cast<const double*>(4096);
    return p;
}

// the camera of either camera argument block: 1 x 4 x 4 frames, 3 stacked, the shortest history n_step 4 allows
template <typename Block>
static void fill_camera(Block& p) {
    uint8_t* frames = reinterpret_cast<uint8_t*>(4096);
    p.C = 1; p.H = 4; p.W = 4; p.frame_stacks = 3; p.hist_len = 7; p.hist_pos = 6;
    p.step_frame_next = frames; p.step_frame_reset = frames;
    p.hist = frames; p.pixel = frames; p.pixel_next = frames; p.obs_pixel = frames;
}

static struct smx_record_ppo_pixel_window_step ppo_pixel(const std::vector<int32_t>& t, const std::vector<int32_t>& rank) {
    struct smx_record_ppo_pixel_window_step p;   // (the tag: the entry point has the same name)
    fill_shared(p, t, rank);
    p.advance = 3; p.step_pds = fake(); p.carry_pd = fake(); p.pds = fake();
    fill_camera(p);
    return p;
}

static struct smx_record_ddpg_pixel_nstep_step ddpg_pixel(const std::vector<int32_t>& t, const std::vector<int32_t>& rank) {
    struct smx_record_ddpg_pixel_nstep_step p;
    fill_shared(p, t, rank);
    p.gpow = reinterpret_cast<const double*>(4096);
    fill_camera(p);
    return p;
}

int main() {
    const std::vector<int32_t> t = {0, 3, 4, 7, 1}, rank = {-1, 0, -1, 1, -1};
    const std::vector<int32_t> t_neg = {0, 3, -1, 7, 1}, rank_big = {-1, 0, -1, 5, -1}, rank_low = {-1, 0, -2, 1, -1};

    expect("ppo: null argument block", smx_record_ppo_window_step_f32(nullptr, nullptr), SMX_E_NULL);
    expect("ddpg: null argument block", smx_record_ddpg_nstep_step_f32(nullptr, nullptr), SMX_E_NULL);
    {
        auto p = ppo(t, rank); p.obs = nullptr;
        expect("ppo: null obs table", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_NULL);
        p = ppo(t, rank); p.pds = nullptr;
        expect("ppo: null pds table", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_NULL);
        p = ppo(t, rank); p.carry_obs = nullptr;
        expect("ppo: null carry ring", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_NULL);
        p = ppo(t, rank); p.rank = nullptr;
        expect("ppo: null rank", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_NULL);
        p = ppo(t, rank); p.h_before = fake();
        expect("ppo: h_before without c_before", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_NULL);
        p = ppo(t, rank); p.mon.ep_reward = reinterpret_cast<double*>(4096);
        expect("ppo: a monitor with one pointer", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_NULL);
        p = ppo(t, rank_big);
        expect("ppo: rank >= n", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ppo(t, rank_low);
        expect("ppo: rank < -1", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ppo(t_neg, rank);
        expect("ppo: t < 0", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ppo(t, rank); p.capacity = 4;
        expect("ppo: n > capacity", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ppo(t, rank); p.rows = 3;
        expect("ppo: rows != closing actors", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ppo(t, rank); p.advance = 5;
        expect("ppo: advance > n_step", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ppo(t, rank); p.cursor = 64;
        expect("ppo: cursor outside the ring", smx_record_ppo_window_step_f32(&p, nullptr), SMX_E_SHAPE);
    }
    {
        auto p = ddpg(t, rank); p.obs_next = nullptr;
        expect("ddpg: null obs_next table", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_NULL);
        p = ddpg(t, rank); p.gpow = nullptr;
        expect("ddpg: null gpow", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_NULL);
        p = ddpg(t, rank); p.t = nullptr;
        expect("ddpg: null t", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_NULL);
        p = ddpg(t, rank_big);
        expect("ddpg: rank >= n", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ddpg(t_neg, rank);
        expect("ddpg: t < 0", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ddpg(t, rank); p.capacity = 4;
        expect("ddpg: n > capacity", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_SHAPE);
        p = ddpg(t, rank); p.n_step = 0;
        expect("ddpg: n_step 0", smx_record_ddpg_nstep_step_f32(&p, nullptr), SMX_E_SHAPE);
    }
    {
        auto p = ppo_pixel(t, rank); p.hist = nullptr;
        expect("ppo pixel: null history", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_NULL);
        p = ppo_pixel(t, rank); p.step_frame_next = nullptr;
        expect("ppo pixel: null step_frame_next", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_NULL);
        p = ppo_pixel(t, rank); p.obs = nullptr;
        expect("ppo pixel: null obs table", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_NULL);
        p = ppo_pixel(t, rank); p.hist_len = 6;
        expect("ppo pixel: hist_len < n_step + frame_stacks", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
        p = ppo_pixel(t, rank); p.hist_pos = 7;
        expect("ppo pixel: hist_pos == hist_len", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
        p = ppo_pixel(t, rank); p.hist_pos = -1;
        expect("ppo pixel: hist_pos < 0", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
        p = ppo_pixel(t, rank); p.capacity = 4;
        expect("ppo pixel: n > capacity", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
        p = ppo_pixel(t, rank); p.rows = 3;
        expect("ppo pixel: rows != closing actors", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
        p = ppo_pixel(t, rank); p.D = 0;
        expect("ppo pixel: D 0 (a pixel-only observation)", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
        p = ppo_pixel(t, rank); p.copy_workgroups = 1025;
        expect("ppo pixel: copy_workgroups > 1024", smx_record_ppo_pixel_window_step(&p, nullptr), SMX_E_SHAPE);
    }
    {
        auto p = ddpg_pixel(t, rank); p.pixel_next = nullptr;
        expect("ddpg pixel: null pixel_next table", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_NULL);
        p = ddpg_pixel(t, rank); p.gpow = nullptr;
        expect("ddpg pixel: null gpow", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_NULL);
        p = ddpg_pixel(t, rank); p.hist_len = 6;
        expect("ddpg pixel: hist_len < n_step + frame_stacks", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_SHAPE);
        p = ddpg_pixel(t, rank); p.hist_pos = 7;
        expect("ddpg pixel: hist_pos == hist_len", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_SHAPE);
        p = ddpg_pixel(t, rank); p.frame_stacks = 0;
        expect("ddpg pixel: frame_stacks 0", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_SHAPE);
        p = ddpg_pixel(t_neg, rank);
        expect("ddpg pixel: t < 0", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_SHAPE);
        p = ddpg_pixel(t, rank); p.copy_workgroups = -1;
        expect("ddpg pixel: copy_workgroups < 0", smx_record_ddpg_pixel_nstep_step(&p, nullptr), SMX_E_SHAPE);
    }
    printf("%d unexpected\n", failures);
    return failures != 0;
}
