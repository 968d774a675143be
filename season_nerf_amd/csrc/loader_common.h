// Integer arithmetic of the device ray loader (csrc/loader.hip), shared with its host mirrors (csrc/api.cpp: snerf_loader_indices_host,
// snerf_loader_sc_rays_host): exact, so host and device produce the same indices and the same sun-check rays bit for bit.
//   loader_perm      keyed bijection of [0, n): balanced Feistel network over 2^bits >= n (bits even), six rounds, murmur3's 32-bit finaliser as the round
//                    function, round keys from (seed, epoch) through splitmix64, cycle-walking while the value is >= n
//   step_inputs_words  the words of the per-step training inputs (sun rays, jitter): Philox under a key of its own; the word assignment is stated there
//   philox4x32_10    Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC 2011); pinned by the known-answer vectors of Random123
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define SNERF_HD __host__ __device__
#else
#define SNERF_HD
#endif

namespace snerf {

constexpr int kLoaderRounds = 6;
constexpr int kLoaderCols = 22;          // Img_Pt 2 | Top 3 | Bot 3 | View_Angle 3 | Sun_Angle 3 | Time_Encoded 4 | Sample_Weight 1 | GT_Color 3

SNERF_HD inline uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}
SNERF_HD inline uint64_t splitmix64(uint64_t z) {
    z += 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
// smallest even number of bits whose range covers n rows (n >= 1): 2 .. 62
SNERF_HD inline int loader_bits(int64_t n) {
    int b = 2;
    while (b < 62 && ((int64_t)1 << b) < n) b += 2;
    return b;
}
struct LoaderKeys { uint32_t k[kLoaderRounds]; };
// the shuffle's stream of the seed: (seed, epoch, round) through two splitmix64 steps; the sun-check rays key Philox with the seed itself
SNERF_HD inline LoaderKeys loader_keys(uint64_t seed, uint64_t epoch) {
    LoaderKeys K;
    const uint64_t base = splitmix64(seed ^ 0x73686f66666c6531ull) ^ splitmix64(epoch);
    for (int r = 0; r < kLoaderRounds; ++r) K.k[r] = (uint32_t)(splitmix64(base + (uint64_t)r) >> 32);
    return K;
}
SNERF_HD inline uint64_t loader_feistel(uint64_t v, int bits, const LoaderKeys& K) {
    const int half = bits >> 1;
    const uint32_t mask = half >= 32 ? 0xffffffffu : ((1u << half) - 1u);
    uint32_t L = (uint32_t)(v >> half) & mask, R = (uint32_t)v & mask;
    for (int r = 0; r < kLoaderRounds; ++r) {
        const uint32_t t = L ^ (fmix32(R ^ K.k[r]) & mask);
        L = R;
        R = t;
    }
    return ((uint64_t)L << half) | R;
}
SNERF_HD inline int64_t loader_perm(int64_t p, int64_t n, int bits, const LoaderKeys& K) {
    uint64_t v = loader_feistel((uint64_t)p, bits, K);
    while (v >= (uint64_t)n) v = loader_feistel(v, bits, K);        // p < n lies on a cycle of the bijection that returns below n
    return (int64_t)v;
}

SNERF_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
// the four words of sun-check ray i of draw `draws` on `rank`: counter (i, draws lo, draws hi, rank), key = the seed's two halves
SNERF_HD inline void loader_sc_words(uint64_t seed, uint64_t draws, uint32_t rank, uint32_t i, uint32_t out[4]) {
    const uint32_t ctr[4] = {i, (uint32_t)draws, (uint32_t)(draws >> 32), rank}, key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32_10(ctr, key, out);
}
// u in [0, 1) from the top 24 bits: exact in fp32
SNERF_HD inline float loader_uniform(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }

// ---- per-step training inputs (step_inputs_draw_kernel of csrc/loader.hip, snerf_step_inputs_words_host of csrc/api.cpp) --------------------------------
// A stream of its own: the key is the two halves of splitmix64(seed ^ kStepInputsTag) - the sun-check rays above key Philox with the seed itself.
// Counter (index, draws lo, draws hi, rank + (block << 24)), rank < 2^24; the word assignment:
//   block 0, index = ray i       w0 azimuth, w1 elevation (all 32 bits: u = w * 2^-32 in float64), w2 start x, w3 start y (top 24 bits: loader_uniform)
//   block 1, index = ray i       w0 first time angle, w1 second time angle (top 24 bits), w2 / w3 unused
//   block 2, index = sample s    w0 jitter of the image pass, w1 jitter of the sun-ray pass (top 24 bits), w2 / w3 unused
constexpr uint64_t kStepInputsTag = 0x73746570696e7031ull;      // "stepinp1"
constexpr uint32_t kStepInputsMaxRank = 1u << 24;
SNERF_HD inline void step_inputs_words(uint64_t seed, uint64_t draws, uint32_t rank, uint32_t block, uint32_t index, uint32_t out[4]) {
    const uint64_t k = splitmix64(seed ^ kStepInputsTag);
    const uint32_t ctr[4] = {index, (uint32_t)draws, (uint32_t)(draws >> 32), rank + (block << 24)}, key[2] = {(uint32_t)k, (uint32_t)(k >> 32)};
    philox4x32_10(ctr, key, out);
}

}  // namespace snerf
