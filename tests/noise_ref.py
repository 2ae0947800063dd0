"""The rollouts' exploration-noise stream (struct smx_noise_stream, include/surreal_amd.h) restated in numpy float64
from its definition.  Tests only.

    x[0..3] = philox4x32_10(counter = (g, low32(s), high32(s), j >> 2), key = (low32(seed), high32(seed)))
    pair p = (j & 3) >> 1:  u0 = ((x[2p] >> 8) + 0.5) 2^-24,  u1 = ((x[2p + 1] >> 8) + 0.5) 2^-24
    r = sqrt(-2 ln u0);  normal = r cos(2 pi u1) for even j, r sin(2 pi u1) for odd j

The ten rounds run on whole arrays here (uint64 lanes holding 32-bit words); `philox_ref.philox4x32_10`, the scalar
restatement the known-answer vectors hold, is what `philox_blocks` is checked against (test_rollout_noise_cpu.py)."""
import numpy as np

from philox_ref import M0, M1, W0, W1, MASK

BOUND = float(np.sqrt(-2.0 * np.log(2.0 ** -25)))        # the largest |normal|: u0 = 2^-25


def philox_blocks(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (broadcast against each other) -> four uint64 arrays of 32-bit words"""
    c = [np.asarray(x, dtype=np.uint64) & np.uint64(MASK) for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    m0, m1, sh, mask = np.uint64(M0), np.uint64(M1), np.uint64(32), np.uint64(MASK)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                    # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def normal(seed, g, s, j):
    """the stream's standard normal for (seed, global actor id g, draw step s, component j), float64; g, s, j arrays
    (broadcast) or integers"""
    g, s, j = np.broadcast_arrays(np.asarray(g, dtype=np.uint64), np.asarray(s, dtype=np.uint64),
                                  np.asarray(j, dtype=np.uint64))
    seed = int(seed)
    x = philox_blocks(g, s & np.uint64(MASK), s >> np.uint64(32), j >> np.uint64(2), seed & MASK, (seed >> 32) & MASK)
    hi = (j & np.uint64(2)) != 0
    x0, x1 = np.where(hi, x[2], x[0]), np.where(hi, x[3], x[1])
    u0 = ((x0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    u1 = ((x1 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u0))
    ang = 2.0 * np.pi * u1
    return np.where((j & np.uint64(1)) != 0, r * np.sin(ang), r * np.cos(ang))


def draws(seed, actor_base, step, T, n, A):
    """[T, n, A] float64: what smx_noise_fill_f32 / DeviceNoise.draws(T, n, A) form in fp32"""
    k = np.arange(T, dtype=np.uint64).reshape(T, 1, 1) + np.uint64(step)
    g = np.arange(n, dtype=np.uint64).reshape(1, n, 1) + np.uint64(actor_base)
    j = np.arange(A, dtype=np.uint64).reshape(1, 1, A)
    return normal(seed, g, k, j)


def moments_ok(z):
    """the issue's three checks on N draws: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N), every |z| <= BOUND ->
    (mean, var, max |z|) after asserting them"""
    z = np.asarray(z, dtype=np.float64).ravel()
    N = z.size
    mean, var, top = float(z.mean()), float(z.var()), float(np.abs(z).max())
    print('noise moments over %d draws: mean %.3e (bound %.3e), var - 1 %.3e (bound %.3e), max |z| %.4f (bound %.4f)'
          % (N, mean, 5 / np.sqrt(N), var - 1, 5 * np.sqrt(2.0 / N), top, BOUND))
    assert abs(mean) <= 5 / np.sqrt(N), mean
    assert abs(var - 1) <= 5 * np.sqrt(2.0 / N), var
    assert top <= BOUND, top
    return mean, var, top
