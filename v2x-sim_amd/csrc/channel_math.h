// Arithmetic of the degraded-link draw (channel.hip): the Philox4x32-10 rounds, the counter layout of a directed pair, the two
// uniforms and the Box-Muller normals.  ONE definition that the kernel and a host driver compile: plain integers and floats in, plain integers and
// floats out -- no HIP type -- so tests/test_channel_math_cpu.py builds it with the host compiler and compares words, uniforms and link decisions bit
// for bit with a reference written from the definitions (tests/channel_refs.py).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define V2X_CHAN_FN __host__ __device__ __forceinline__
#else
#define V2X_CHAN_FN static inline
#endif

constexpr int CHAN_MAX_AGENTS = 32;      // the agent indices have 8 bits each in the counter; the build stops at 32
constexpr uint32_t CHAN_DOMAIN_OUTAGE = 0, CHAN_DOMAIN_POSE = 1;

struct ChanWords { uint32_t w[4]; };

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC 2011): ten rounds, the key bumped between them
V2X_CHAN_FN ChanWords chan_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += W0;
        k1 += W1;
    }
    return {{c0, c1, c2, c3}};
}

// the four words of the directed pair (ego i, source j) of frame f at step s: nothing else enters a draw
V2X_CHAN_FN ChanWords chan_words(uint64_t seed, uint64_t step, uint32_t frame, uint32_t domain, uint32_t ego, uint32_t src) {
    return chan_philox4x32_10((uint32_t)step, (uint32_t)(step >> 32), frame, (domain << 16) | (ego << 8) | src, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// [0, 1) in steps of 2^-24 and (0, 1) in steps of 2^-23: both exact in fp32
V2X_CHAN_FN float chan_uniform24(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-8f; }
V2X_CHAN_FN float chan_uniform23(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-7f; }

V2X_CHAN_FN bool chan_link_down(const ChanWords &d, float p_outage) { return chan_uniform24(d.w[0]) < p_outage; }

// Box-Muller on the four words of the pose domain; libm's logf / sinf / cosf, no fast forms
V2X_CHAN_FN void chan_normals(const ChanWords &d, float n[3]) {
    const float ua = chan_uniform23(d.w[0]), ub = chan_uniform23(d.w[1]), uc = chan_uniform23(d.w[2]), ud = chan_uniform23(d.w[3]);
    const float ra = sqrtf(-2.0f * logf(ua)), rc = sqrtf(-2.0f * logf(uc));
    const float ta = 6.283185307179586f * ub, tc = 6.283185307179586f * ud;
    n[0] = ra * cosf(ta);
    n[1] = ra * sinf(ta);
    n[2] = rc * cosf(tc);
}
