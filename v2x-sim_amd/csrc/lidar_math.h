// Arithmetic of the LiDAR ray cast's draw (lidar_cast.hip): the counter layout of a ray and the use of the four Philox words
// -- drop decision, range-noise normal, intensity.  The generator and the two uniforms are channel_math.h's, unchanged.  ONE definition that the
// kernel and a host driver compile: plain integers and floats in, plain integers and floats out -- no HIP type -- so tests/test_lidar_refs_cpu.py
// builds it with the host compiler (tests/lidar_driver.cpp) and compares words, uniforms and drop decisions bit for bit with tests/lidar_refs.py.
// At the end: the three expressions a MOVING scene adds to the geometry, in plain doubles, with a host driver of their own (tests/lidar_motion_driver.cpp).
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

// ---- moving scenes (DESIGN.md section 3.12 "moving scenes"): the three expressions that are new against the static rule, in plain doubles, every product
// and sum rounded on its own (the kernel's file and the host driver tests/lidar_motion_driver.cpp are both compiled with -ffp-contract=off)
// the time of a ray: the start of its sweep plus the offset of its azimuth step
V2X_CHAN_FN double lidar_ray_time(float time_of, float az_time) { return (double)time_of + (double)az_time; }

// a box-frame coordinate of the sensor origin at time T: l0 at time 0, dl the relative velocity (sensor minus box) rotated into the box's frame
V2X_CHAN_FN double lidar_moved(double l0, double dl, double T) {
    const double step = dl * T;
    return l0 + step;
}

// one world-frame component of a box centre relative to the sensor at time T: c0, o0 the positions at time 0, vg, vs the velocities
V2X_CHAN_FN double lidar_rel_centre(double c0, double o0, double vg, double vs, double T) {
    const double e0 = c0 - o0, dv = vg - vs;
    const double step = dv * T;
    return e0 + step;
}
