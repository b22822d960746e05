// rng.hip.h - the counter-based random draws every generator of the library shares (csi_synth_white, the training step's
// noise / dropout / Glorot streams, csi_synth_structured): a draw is a pure function of (stream key, index), so a value does not
// depend on the launch shape or on which call produces it.  tests/train_streams.py replays these formulas on the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace csi {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// uniform in (0,1) and standard normal from a counter (stream, index)
__device__ __forceinline__ float tr_uniform(uint64_t stream, uint64_t idx) {
    const uint64_t h = splitmix64(stream ^ splitmix64(idx));
    return ((float)(uint32_t)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float tr_normal(uint64_t stream, uint64_t idx) {
    const uint64_t h = splitmix64(stream ^ splitmix64(idx));
    const float u1 = ((float)(uint32_t)(h >> 32) + 0.5f) * (1.0f / 4294967296.0f);
    const float u2 = ((float)(uint32_t)h + 0.5f) * (1.0f / 4294967296.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);
}

}  // namespace csi
