// Layer-1 K loop of the fused critic pass (smx_mlp3_rows16.hip) in both arithmetics -- fp32 MFMA (16x16x4) and
// three-way split bf16 (six 16x16x32 products per tile) -- at the pass's real footprint: 8 wavefronts per workgroup,
// 2 per SIMD, 19 feature tiles, 12 K chunks, weights staged through LDS from the L2-resident packed image, x from
// global memory, 1024 workgroups over all CUs.  The loops are the kernel's own (a copy would drift): this program
// links the two kernel sources with the phase stamps compiled in and reads layer 1's cycles from them.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -DSMX_FUSED_TIMING -Iinclude \
//       scripts/micro/critic_split_loop.hip surreal_amd/csrc/smx_mlp3_fused.hip surreal_amd/csrc/smx_mlp3_rows16.hip \
//       -o critic_split_loop
//   ./critic_split_loop [rows]          (random data; stdout is what profiles/critic_split_loop.txt records)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "surreal_amd.h"

extern "C" void smx_mlp3_fused_debug_tbuf(void* p);

#define CK(e) do { hipError_t e_ = (e); if (e_ != hipSuccess) { printf("HIP error %d at line %d\n", (int)e_, __LINE__); return 1; } } while (0)
#define RC(e) do { int r_ = (e); if (r_) { printf("library error %d at line %d\n", r_, __LINE__); return 1; } } while (0)

static unsigned lcg_state = 12345u;
static float urand() { lcg_state = lcg_state * 1664525u + 1013904223u; return (float)(lcg_state >> 8) * (1.0f / 16777216.0f); }
static float nrand() { float s = 0.f; for (int i = 0; i < 12; ++i) s += urand(); return s - 6.0f; }

static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
    const int D = 376, H1 = 300, H2 = 200, OUT = 1, KC = (D + 31) / 32;
    const long rows = argc > 1 ? atol(argv[1]) : 131072;
    const long wgs = (rows + 127) / 128;
    std::vector<float> hx((size_t)rows * D), hw((size_t)H1 * D + H1 + (size_t)H2 * H1 + H2 + H2 + 1), hzm(D), hzs(D);
    for (auto& v : hx) v = nrand();
    {
        size_t i = 0;
        const float s1 = 1.0f / sqrtf((float)D), s2 = 1.0f / sqrtf((float)H1), s3 = 1.0f / sqrtf((float)H2);
        for (; i < (size_t)H1 * D + H1; ++i) hw[i] = (2.f * urand() - 1.f) * s1;
        for (const size_t e = i + (size_t)H2 * H1 + H2; i < e; ++i) hw[i] = (2.f * urand() - 1.f) * s2;
        for (; i < hw.size(); ++i) hw[i] = (2.f * urand() - 1.f) * s3;
    }
    for (int k = 0; k < D; ++k) { hzm[k] = 0.1f * nrand(); hzs[k] = 0.5f + urand(); }
    float *x, *w, *zm, *zs, *packed, *out0, *out1;
    long long* tbuf;
    CK(hipMalloc(&x, hx.size() * 4)); CK(hipMalloc(&w, hw.size() * 4)); CK(hipMalloc(&zm, D * 4)); CK(hipMalloc(&zs, D * 4));
    CK(hipMalloc(&out0, rows * 4)); CK(hipMalloc(&out1, rows * 4)); CK(hipMalloc(&tbuf, wgs * 16 * 8));
    CK(hipMemcpy(x, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(w, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(zm, hzm.data(), D * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(zs, hzs.data(), D * 4, hipMemcpyHostToDevice));
    smx_mlp3_t net;
    net.W1 = w; net.b1 = net.W1 + (size_t)H1 * D; net.W2 = net.b1 + H1; net.b2 = net.W2 + (size_t)H2 * H1;
    net.W3 = net.b2 + H2; net.b3 = net.W3 + H2;
    net.D = D; net.H1 = H1; net.H2 = H2; net.OUT = OUT;
    const size_t pbytes = smx_mlp3_packed_bytes(D, H1, H2, OUT);
    CK(hipMalloc(&packed, pbytes));
    RC(smx_mlp3_pack_f32(&net, packed, pbytes, nullptr));
    CK(hipDeviceSynchronize());

    float* outs[2] = {out0, out1};
    double l1[2] = {0, 0};
    for (int split = 0; split < 2; ++split) {
        auto launch = [&]() {
            return smx_mlp3_forward_fused_split_f32(packed, pbytes, split, D, H1, H2, OUT, x, nullptr, rows, 1, 0, zm, zs,
                                                    outs[split], SMX_ACT_NONE, nullptr);
        };
        smx_mlp3_fused_debug_tbuf(nullptr);
        for (int i = 0; i < 10; ++i) RC(launch());
        CK(hipDeviceSynchronize());
        hipEvent_t e0, e1;
        CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        const int n = 30;
        CK(hipEventRecord(e0, 0));
        for (int i = 0; i < n; ++i) RC(launch());
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms = 0.f;
        CK(hipEventElapsedTime(&ms, e0, e1));
        CK(hipMemset(tbuf, 0, wgs * 16 * 8));
        smx_mlp3_fused_debug_tbuf(tbuf);
        RC(launch());                      // right behind the timed launches: the same clocks
        CK(hipDeviceSynchronize());
        smx_mlp3_fused_debug_tbuf(nullptr);
        std::vector<long long> t(wgs * 16);
        CK(hipMemcpy(t.data(), tbuf, wgs * 16 * 8, hipMemcpyDeviceToHost));
        std::vector<double> ph[5], tot;
        for (long b = 0; b < wgs; ++b) {
            for (int i = 0; i < 5; ++i) ph[i].push_back((double)(t[b * 16 + i + 1] - t[b * 16 + i]));
            tot.push_back((double)(t[b * 16 + 5] - t[b * 16]));
        }
        l1[split] = median(ph[1]);
        printf("%s: %.1f us per launch (back to back, %ld rows); workgroup cycles, median over %ld: prologue %.0f  "
               "layer 1 %.0f  hand-over %.0f  layer 2 %.0f  epilogue %.0f  total %.0f\n",
               split ? "split bf16 (6 products)" : "fp32 MFMA            ", ms * 1e3 / n, rows, wgs, median(ph[0]),
               median(ph[1]), median(ph[2]), median(ph[3]), median(ph[4]), median(tot));
        printf("    layer-1 loop: %.0f cycles per 32-wide K chunk (%d chunks)\n", l1[split] / KC, KC);
    }
    printf("fp32 / split cycles per chunk: %.2f x  (stop rule: at least 1.4 x)\n", l1[0] / l1[1]);
    std::vector<float> o0(rows), o1(rows);
    CK(hipMemcpy(o0.data(), out0, rows * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(o1.data(), out1, rows * 4, hipMemcpyDeviceToHost));
    double mx = 0, sum = 0, amax = 0;
    for (long i = 0; i < rows; ++i) {
        const double d = fabs((double)o0[i] - (double)o1[i]);
        if (!(d <= mx)) mx = d;
        sum += d;
        amax = std::max(amax, (double)fabsf(o0[i]));
    }
    printf("outputs, split against fp32: max |diff| %.3g  mean %.3g  (max |out| %.3g)\n", mx, sum / rows, amax);
    return 0;
}
