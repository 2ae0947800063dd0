// The LSTM gate non-linearities of smx_lstm.hip's default kernels, shared with the persistent LSTM rollout
// (smx_rollout.hip) so that both form the same gates.  Included inside an anonymous namespace.
#pragma once

// Gate non-linearities on the hardware exp2 / rcp units.  A step of the one-row recurrence lasts as long as ONE wavefront
// needs for its own in-order instruction stream (profiles/r03_pmc_lstm.json: vector ALUs 24 % busy, LDS 2 % -- nothing is
// saturated), and more than half of that stream was the libm expf / tanhf / IEEE division of sigmoid and tanh -- on
// BOTH sides of the tanh-or-sigmoid branch, since the four gates of a unit sit in one quad.  sigmoid(z) = rcp(1 +
// exp2(-z log2 e)) is 5 instructions; tanh(x) = 2 sigmoid(2 x) - 1 shares them, so a lane's gate is ONE branch-free
// sequence.  Absolute error <= 1.5e-7 (v_exp_f32 and v_rcp_f32 are 1 ulp; the argument scaling adds |z| 2^-24 relative
// to an exponent whose sensitivity s (1 - s) |z| peaks at 0.22) against the 1e-5 parity bound.
__device__ __forceinline__ float fast_sigm(float z) {
    return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896341f * z));
}
__device__ __forceinline__ float fast_tanh(float x) { return 2.f * fast_sigm(2.f * x) - 1.f; }
