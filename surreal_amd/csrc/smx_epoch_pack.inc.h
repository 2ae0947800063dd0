// The packed weight layout of the fused epoch kernels (smx_epoch.hip), shared with the optimiser kernel
// (smx_ppo.hip) that keeps it current.  Included inside an anonymous namespace.
//
// A matrix X [M, K] (a layer's weights, or their transpose for the backward kernel) is stored as
// [tile of 16 rows][32-wide K chunk][half][lane][4 floats], zero padded to whole tiles and an EVEN
// number of chunks: lane l = 16 kq + i of (tile t, chunk c, half h) holds X[16 t + i][32 c + 8 kq + 4 h + 0..3]
// -- the A operands of four consecutive v_mfma_f32_16x16x4_f32 steps, one contiguous KB per load
// instruction.  A net's copy is [W1 | W2 | W3 | W2^T | W3^T].
#pragma once

__host__ __device__ inline int pack_chunks(int K) { return (((K + 31) >> 5) + 1) & ~1; }
__host__ __device__ inline long pack_words(int M, int K) {       // 16-byte words of one packed block
    return (long)((M + 15) >> 4) * pack_chunks(K) * 128;
}
__host__ __device__ inline long pack_off(int D, int H1, int H2, int OUT, int blockno) {   // in 16-byte words
    long o = 0;
    if (blockno > 0) o += pack_words(H1, D);
    if (blockno > 1) o += pack_words(H2, H1);
    if (blockno > 2) o += pack_words(OUT, H2);
    if (blockno > 3) o += pack_words(H1, H2);
    if (blockno > 4) o += pack_words(H2, OUT);
    return o;
}
// float index of X[m][k] inside its packed block
__host__ __device__ inline long pack_pos(int K, int m, int k) {
    const int kk = k & 31;
    const long word = ((long)((m >> 4) * pack_chunks(K) + (k >> 5)) * 2 + ((kk >> 2) & 1)) * 64 + (kk >> 3) * 16 + (m & 15);
    return word * 4 + (kk & 3);
}

// 16-byte word w of a net's copy: block bn, and the four elements X[m][k .. k + 3] of its matrix X [M, K] it holds
// (zeros past M or K) -- the layer's weights, or (tr) their transpose: X[m][k] = W[k][m], W [K, M]
struct PackSrc {
    int bn, M, K, m, k;
    bool tr;
};
__host__ __device__ inline PackSrc pack_decode(int D, int H1, int H2, int OUT, long w) {
    PackSrc s;
    s.bn = 0;
#pragma unroll
    for (int b = 1; b < 5; ++b) s.bn += (w >= pack_off(D, H1, H2, OUT, b)) ? 1 : 0;
    w -= pack_off(D, H1, H2, OUT, s.bn);
    s.tr = s.bn >= 3;
    s.M = s.bn == 0 ? H1 : (s.bn == 1 ? H2 : (s.bn == 2 ? OUT : (s.bn == 3 ? H1 : H2)));
    s.K = s.bn == 0 ? D : (s.bn == 1 ? H1 : (s.bn == 2 ? H2 : (s.bn == 3 ? H2 : OUT)));
    const int C2 = pack_chunks(s.K);
    const int lane = (int)(w & 63), half = (int)((w >> 6) & 1);
    const long tc = w >> 7;
    const int c = (int)(tc % C2), t = (int)(tc / C2);
    s.m = 16 * t + (lane & 15);
    s.k = 32 * c + 8 * (lane >> 4) + 4 * half;
    return s;
}

// One agent's copy in a population of perturbed actors (smx_param_noise_refresh_f32 writes them, the population
// rollout of smx_rollout.hip reads them): [the net's copy above | b1 | b2 | b3], rounded up to 64 floats
__host__ __device__ inline long pop_bias_off(int D, int H1, int H2, int OUT) { return 4 * pack_off(D, H1, H2, OUT, 5); }
__host__ __device__ inline long pop_copy_floats(int D, int H1, int H2, int OUT) {
    return (pop_bias_off(D, H1, H2, OUT) + H1 + H2 + OUT + 63) & ~63L;
}
// The copy of a LayerNorm actor (smx_param_noise_refresh_f32 with ln): [the net's copy | b1 | b2 | b3 | ln1.W | ln1.b | ln2.W |
// ln2.b], rounded up to 64 floats
__host__ __device__ inline long pop_ln_off(int D, int H1, int H2, int OUT) { return pop_bias_off(D, H1, H2, OUT) + H1 + H2 + OUT; }
__host__ __device__ inline long pop_ln_copy_floats(int D, int H1, int H2, int OUT) {
    return (pop_ln_off(D, H1, H2, OUT) + 2 * (H1 + H2) + 63) & ~63L;
}
