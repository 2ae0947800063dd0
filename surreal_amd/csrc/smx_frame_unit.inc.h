// The unit the camera launches move frames in (smx_rollout.hip's synthetic camera steps, smx_record.hip's recorder):
// U bytes between global memory and a lane's registers -- 16: one uint4 access (frame sizes that are multiples of 16
// bytes, every frame buffer on 16 bytes), 1: single bytes.  Included inside an anonymous namespace.
#pragma once

template <int U>
__device__ __forceinline__ void store_unit(unsigned char* dst, const unsigned char* b) {
    if constexpr (U == 16) {
        *(uint4*)dst = *(const uint4*)b;
    } else {
#pragma unroll
        for (int i = 0; i < U; ++i) dst[i] = b[i];
    }
}

template <int U>
__device__ __forceinline__ void load_unit(const unsigned char* src, unsigned char* b) {
    if constexpr (U == 16) {
        *(uint4*)b = *(const uint4*)src;
    } else {
#pragma unroll
        for (int i = 0; i < U; ++i) b[i] = src[i];
    }
}
