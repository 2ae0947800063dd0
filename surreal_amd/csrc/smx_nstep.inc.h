// The n-step reward of DDPG's transitions: the one definition every kernel that closes a transition uses
// (smx_rollout.hip's DDPG rollouts and step launches, smx_record.hip's recorder).  Included inside an anonymous
// namespace.  The expression keeps its evaluation order: the build does not contract, and the tests pin these bits.

// the closing transition's reward: r_j + g[e] r_{j+1} + ..., left to right in fp64 (the host wrapper's `+=` sequence),
// exponents as ExpSenderWrapperSSARNStepBootstrap._discount_exponent (the reference's ramp-up quirk included)
__device__ __forceinline__ float nstep_reward(const float* crew_a, const double* gpow, int N, int tau) {
    const int j = tau - N + 1;
    double R = (double)crew_a[j % N];
    for (int u = j + 1; u <= tau; ++u) {
        const int e = (u >= N - 1) ? (u - j) : (N - 1 - j);
        R = R + gpow[e] * (double)crew_a[u % N];
    }
    return (float)R;
}
