// Parameter-space exploration noise on the device (surreal/agent/param_noise.py; Plappert et al., arXiv 1706.01905):
// a population of perturbed actors, one per AGENT -- a group of consecutive actors of a launch that share one
// perturbation, as the actors of one reference agent process do (ddpg_agent.py:136-153).
//
// The perturbation is a pure function (smx_philox.inc.h, param_noise_normal): for global agent id g, generation q and
// element i of the actor's flat parameters
//     W1 [H1, D] | b1 [H1] | W2 [H2, H1] | b2 [H2] | W3 [A, H2] | b3 [A]        (row-major each: DDPGModel's order)
// the perturbed value is  w_i + (float)sigma_g * z(seed, g, q, i)  in fp32, the product first (the build does not
// contract).  The clean parameters are read, never written.
//
//   smx_param_noise_fill_f32     one agent's perturbed flat parameters [numel]
//   smx_param_noise_refresh_f32  on_parameter_fetched for all P agents without a host synchronisation, in at most two
//                                launches: (adaptive, acts > 0) sigma_p <- dist_p / acts > target ? sigma_p / alpha :
//                                sigma_p * alpha in fp64 (param_noise.py:65-70) in a launch of its own, so that the next
//                                one reads finished sigmas; then every agent's copy [smx_epoch_pack_f32's layout of the
//                                perturbed weights | b1 | b2 | b3] (smx_epoch_pack.inc.h, pop_copy_floats) into
//                                packed_pop + p * packed_stride.  Noise goes to logical elements only: the layout's
//                                padding is written as zeros.
//   A LayerNorm actor (pn->ln): the flat parameters go on with ln1.W [H1] | ln1.b [H1] | ln2.W [H2] | ln2.b [H2]
//                                (DDPGModel's order), perturbed by the same rule under their own indices i, and an
//                                agent's copy carries the perturbed four behind its biases (pop_ln_copy_floats).  The
//                                indices of the first six arrays are what they are without a LayerNorm.
#include "smx_common.h"

namespace {
#include "smx_epoch_pack.inc.h"
#include "smx_philox.inc.h"

struct PNArgs {
    const float *W1, *b1, *W2, *b2, *W3, *b3;
    const float* ln;                             // ln1.W | ln1.b | ln2.W | ln2.b behind b3, or null: no LayerNorm
    int D, H1, H2, A;
    uint64_t seed;
    uint32_t g0, q;                              // global id of agent 0, generation
    const double* sigma;                         // [agents]
    float* pop;
    long stride;                                 // floats between two agents' copies
};

// flat offsets of the six arrays, the LayerNorm block behind them (nln of its elements: 0 without one)
struct Flat {
    unsigned b1, W2, b2, W3, b3, ln, nln, numel;
    __host__ __device__ Flat(int D, int H1, int H2, int A, bool with_ln) {
        b1 = (unsigned)H1 * D; W2 = b1 + H1; b2 = W2 + (unsigned)H2 * H1; W3 = b2 + H2; b3 = W3 + (unsigned)A * H2;
        ln = b3 + A;
        nln = with_ln ? 2u * (unsigned)(H1 + H2) : 0u;
        numel = ln + nln;
    }
    __host__ __device__ Flat(const PNArgs& P) : Flat(P.D, P.H1, P.H2, P.A, P.ln != nullptr) {}
};

__device__ __forceinline__ float clean_at(const PNArgs& P, const Flat& F, unsigned i) {
    if (i < F.b1) return P.W1[i];
    if (i < F.W2) return P.b1[i - F.b1];
    if (i < F.b2) return P.W2[i - F.W2];
    if (i < F.W3) return P.b2[i - F.b2];
    if (i < F.b3) return P.W3[i - F.W3];
    if (i < F.ln) return P.b3[i - F.b3];
    return P.ln[i - F.ln];
}

// element i of agent p's perturbed parameters (sg = (float)sigma_p)
__device__ __forceinline__ float perturbed_at(const PNArgs& P, const Flat& F, int p, float sg, unsigned i) {
    return clean_at(P, F, i) + sg * param_noise_normal(P.seed, P.g0 + (uint32_t)p, P.q, i);
}

__global__ __launch_bounds__(256) void param_noise_fill_kernel(PNArgs P, int p, float* __restrict__ out) {
    const Flat F(P);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < F.numel) out[i] = perturbed_at(P, F, p, (float)P.sigma[p], i);
}

__global__ __launch_bounds__(256) void param_noise_adapt_kernel(double* __restrict__ sigma, const double* __restrict__ dist,
                                                                int agents, double acts, double alpha, double target) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= agents) return;
    const double s = sigma[p];
    sigma[p] = (dist[p] / acts > target) ? s / alpha : s * alpha;
}

// grid (words of one copy / 256, agents): thread = one 16-byte word of agent blockIdx.y's copy
__global__ __launch_bounds__(256) void param_noise_pack_kernel(PNArgs P) {
    const Flat F(P);
    const int p = blockIdx.y;
    const long w = (long)blockIdx.x * 256 + threadIdx.x;
    const long pw = pack_off(P.D, P.H1, P.H2, P.A, 5);
    const long total = (P.ln ? pop_ln_copy_floats(P.D, P.H1, P.H2, P.A) : pop_copy_floats(P.D, P.H1, P.H2, P.A)) / 4;
    if (w >= total) return;
    const float sg = (float)P.sigma[p];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (w < pw) {
        const PackSrc s = pack_decode(P.D, P.H1, P.H2, P.A, w);
        const unsigned base = s.bn == 0 ? 0u : ((s.bn == 1 || s.bn == 3) ? F.W2 : F.W3);
        if (s.m < s.M) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (s.k + r < s.K)
                    v[r] = perturbed_at(P, F, p, sg, base + (s.tr ? (unsigned)(s.k + r) * s.M + s.m
                                                                  : (unsigned)s.m * s.K + s.k + r));
        }
    } else {
        // the biases behind the packed blocks, the LayerNorm block behind them: element e of [b1 | b2 | b3 | ln]
        const int nb = P.H1 + P.H2 + P.A;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = (int)(4 * (w - pw)) + r;
            if (e < nb + (int)F.nln)
                v[r] = perturbed_at(P, F, p, sg, e < P.H1 ? F.b1 + e : (e < P.H1 + P.H2 ? F.b2 + (e - P.H1)
                                                                        : (e < nb ? F.b3 + (e - P.H1 - P.H2)
                                                                                  : F.ln + (e - nb))));
        }
    }
    *(float4*)(P.pop + (size_t)p * P.stride + 4 * w) = make_float4(v[0], v[1], v[2], v[3]);
}

// what every entry point asks of the block and takes from it
int fill_args(const struct smx_param_noise* a, PNArgs& P) {
    SMX_REQUIRE(a && a->net && a->sigma, SMX_E_NULL);
    const smx_mlp3_t& n = *a->net;
    SMX_REQUIRE(n.W1 && n.b1 && n.W2 && n.b2 && n.W3 && n.b3, SMX_E_NULL);
    SMX_REQUIRE(n.D > 0 && n.H1 > 0 && n.H2 > 0 && n.OUT > 0 && a->agents > 0, SMX_E_SHAPE);
    SMX_REQUIRE((long long)n.H1 * n.D + (long long)n.H2 * n.H1 + (long long)n.OUT * n.H2 + n.H1 + n.H2 + n.OUT +
                    (a->ln ? 2LL * (n.H1 + n.H2) : 0) < (1LL << 31), SMX_E_SHAPE);
    // every global agent id and the generation in [0, 2^32): one counter word each
    SMX_REQUIRE(a->agent_base >= 0 && a->agent_base + a->agents <= (1LL << 32), SMX_E_SHAPE);
    SMX_REQUIRE(a->generation >= 0 && a->generation < (1LL << 32), SMX_E_SHAPE);
    P.ln = a->ln;
    P.W1 = n.W1; P.b1 = n.b1; P.W2 = n.W2; P.b2 = n.b2; P.W3 = n.W3; P.b3 = n.b3;
    P.D = n.D; P.H1 = n.H1; P.H2 = n.H2; P.A = n.OUT;
    P.seed = a->seed; P.g0 = (uint32_t)a->agent_base; P.q = (uint32_t)a->generation;
    P.sigma = a->sigma; P.pop = a->packed_pop; P.stride = (long)a->packed_stride;
    return SMX_OK;
}

}  // namespace

extern "C" int64_t smx_param_noise_copy_floats(int32_t D, int32_t H1, int32_t H2, int32_t A, int32_t ln) {
    if (D <= 0 || H1 <= 0 || H2 <= 0 || A <= 0) return 0;
    return ln ? pop_ln_copy_floats(D, H1, H2, A) : pop_copy_floats(D, H1, H2, A);
}

extern "C" int smx_param_noise_fill_f32(const struct smx_param_noise* a, int32_t p, float* out, smx_stream_t stream) {
    PNArgs P;
    const int rc = fill_args(a, P);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(out, SMX_E_NULL);
    SMX_REQUIRE(p >= 0 && p < a->agents, SMX_E_SHAPE);
    const Flat F(P);
    hipLaunchKernelGGL(param_noise_fill_kernel, dim3((F.numel + 255) / 256), dim3(256), 0, smx_s(stream), P, (int)p, out);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}

extern "C" int smx_param_noise_refresh_f32(const struct smx_param_noise* a, smx_stream_t stream) {
    PNArgs P;
    const int rc = fill_args(a, P);
    if (rc != SMX_OK) return rc;
    SMX_REQUIRE(a->packed_pop, SMX_E_NULL);
    SMX_REQUIRE(a->agents <= 65535 && a->acts >= 0, SMX_E_SHAPE);
    const long copy = smx_param_noise_copy_floats(P.D, P.H1, P.H2, P.A, a->ln != nullptr);
    SMX_REQUIRE(a->packed_stride >= copy && a->packed_stride % 4 == 0, SMX_E_SHAPE);
    SMX_REQUIRE(((uintptr_t)a->packed_pop & 15) == 0, SMX_E_ALIGN);
    if (a->adaptive && a->acts > 0) {
        SMX_REQUIRE(a->dist, SMX_E_NULL);
        hipLaunchKernelGGL(param_noise_adapt_kernel, dim3((a->agents + 255) / 256), dim3(256), 0, smx_s(stream), a->sigma,
                           a->dist, a->agents, (double)a->acts, a->alpha, a->target);
        SMX_LAUNCH_CHECK();
    }
    const long words = copy / 4;
    hipLaunchKernelGGL(param_noise_pack_kernel, dim3((unsigned)((words + 255) / 256), a->agents), dim3(256), 0,
                       smx_s(stream), P);
    SMX_LAUNCH_CHECK();
    return SMX_OK;
}
