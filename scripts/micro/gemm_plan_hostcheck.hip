// Stand-alone host check of the dense layer's planner (csrc/smx_gemm.hip: plan_batch and wgrad_batch_takes_tiles): reads
// problem lists, prints the kernel and the grid the library would launch for each, and launches nothing -- so it runs on a
// machine without a GPU, and under the host sanitizers.  The planner has no public symbol: this file includes the
// translation unit.
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       scripts/micro/gemm_plan_hostcheck.hip surreal_amd/csrc/smx_wgrad.hip surreal_amd/csrc/smx_mlp3_bwd16.hip \
//       -o scripts/micro/gemm_plan_hostcheck
//   python scripts/check_gemm_plan.py      # feeds the tests' case table and compares with tests/dense_cases.py
// Input (stdin): `list <id> <n>` followed by n lines `M N K a_kc lda a_off b_kc ldb b_off dbias splits k_chunk`, the
// fields of dense_cases.Prob.  The operands are fake pointers, 16-byte aligned plus 4 * off bytes, never dereferenced.
// Output: one line per list, `<id> <kernel> <grid> <1 when wgrad_batch_takes_tiles>`, or `<id> refused <code>`.
#include "../../surreal_amd/csrc/smx_gemm.hip"
#include <stdio.h>

static float* fake(int off_floats) { return reinterpret_cast<float*>((uintptr_t)(1 << 20) + 4u * (unsigned)off_floats); }

int main() {
    char id[128];
    int n, lists = 0;
    while (scanf(" list %127s %d", id, &n) == 2) {
        if (n < 1 || n > MAX_PROBS) {
            fprintf(stderr, "%s: %d problems\n", id, n);
            return 2;
        }
        GemmBatch G;
        G.n = n;
        for (int k = 0; k < n; ++k) {
            int M, N, K, a_kc, lda, a_off, b_kc, ldb, b_off, dbias, splits, k_chunk;
            if (scanf("%d %d %d %d %d %d %d %d %d %d %d %d", &M, &N, &K, &a_kc, &lda, &a_off, &b_kc, &ldb, &b_off, &dbias,
                      &splits, &k_chunk) != 12) {
                fprintf(stderr, "%s: problem %d is not 12 integers\n", id, k);
                return 2;
            }
            GemmProb& P = G.p[k];
            P = gemm_prob(fake(a_off), lda, a_kc, fake(b_off), ldb, b_kc, fake(0), N, M, N, K);
            if (dbias) P.dbias = fake(0);
            if (splits > 1) split_prob(P, SplitK{k_chunk, splits});
        }
        const bool tiles = wgrad_batch_takes_tiles(G);
        GemmPlan plan;
        const int rc = plan_batch(G, plan);
        if (rc) {
            printf("%s refused %d\n", id, rc);
        } else {
            char name[16];
            if (plan.kernel == GEMM_TILE) snprintf(name, sizeof(name), "tile%d%d", plan.am, plan.bm);
            else snprintf(name, sizeof(name), "%s", plan.kernel == GEMM_ROWS ? "rows" : plan.kernel == GEMM32_CO ? "gemm32_co" : "gemm32");
            // the tiles as numbered: each problem's base is the sum of the counts in front of it, the grid their total
            int base = 0;
            for (int k = 0; k < n; ++k) {
                if (G.p[k].tile_base != base) {
                    fprintf(stderr, "%s: problem %d starts at tile %d, not %d\n", id, k, G.p[k].tile_base, base);
                    return 3;
                }
                base += G.p[k].tiles_m * G.p[k].tiles_n * G.p[k].splits;
            }
            if (base != plan.grid) {
                fprintf(stderr, "%s: grid %d, tiles %d\n", id, plan.grid, base);
                return 3;
            }
            printf("%s %s %d %d\n", id, name, plan.grid, tiles ? 1 : 0);
        }
        ++lists;
    }
    fprintf(stderr, "%d lists\n", lists);
    return lists ? 0 : 2;
}
