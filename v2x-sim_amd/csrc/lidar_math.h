// Arithmetic of the LiDAR ray cast's draw (lidar_cast.hip): the counter layout of a ray and the use of the four Philox words
// -- drop decision, range-noise normal, intensity.  The generator and the two uniforms are channel_math.h's, unchanged.  ONE definition that the
// kernel and a host driver compile: plain integers and floats in, plain integers and floats out -- no HIP type -- so tests/test_lidar_refs_cpu.py
// builds it with the host compiler (tests/lidar_driver.cpp) and compares words, uniforms and drop decisions bit for bit with tests/lidar_refs.py.
#pragma once
#include "channel_math.h"

constexpr uint32_t LIDAR_DOMAIN = 0x4C440000u;      // "LD" in the top half of the fourth counter word; the low half takes bits 32..47 of the step

// the four words of ray r of sweep s at step `step`: nothing else enters a draw (not sigma_r, not p_drop, not the launch geometry)
V2X_CHAN_FN ChanWords lidar_words(uint64_t seed, uint64_t step, uint32_t sweep, uint32_t ray) {
    return chan_philox4x32_10(ray, sweep, (uint32_t)step, LIDAR_DOMAIN | (uint32_t)((step >> 32) & 0xffffu), (uint32_t)seed, (uint32_t)(seed >> 32));
}

// word 0: the return is lost
V2X_CHAN_FN bool lidar_dropped(const ChanWords &d, float p_drop) { return chan_uniform24(d.w[0]) < p_drop; }

// words 1 and 2: one standard normal by Box-Muller; libm's logf / cosf, no fast forms (chan_normals' first component on other words)
V2X_CHAN_FN float lidar_normal(const ChanWords &d) {
    const float ua = chan_uniform23(d.w[1]), ub = chan_uniform23(d.w[2]);
    return sqrtf(-2.0f * logf(ua)) * cosf(6.283185307179586f * ub);
}

// word 3: the intensity in [0, 1)
V2X_CHAN_FN float lidar_intensity(const ChanWords &d) { return chan_uniform24(d.w[3]); }

// the range a return reports: noise after the choice of the winner and after the range check
V2X_CHAN_FN float lidar_noisy_range(double t, float sigma_r, float nrm) { return fmaf(sigma_r, nrm, (float)t); }
