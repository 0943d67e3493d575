// The communication codec of `compress_level = k` as ONE streaming kernel: upstream's com_compresser / bn_compress / com_decompresser / bn_decompress around the
// transmitted 256-channel map (coperception Backbone.py::LidarEncoder with compress_level > 0 -- code absent from the reference tree, frozen in DESIGN.md section 3):
//     msg = relu(bn_c(Wc x))   [Cc = C >> k channels, the bytes an agent SENDS]        y = relu(bn_d(Wd msg))   [C channels]
// Two 1x1 layers, i.e. two pure per-pixel streams (conv1x1.hip), with an intermediate of 2^-k of the map.  As two launches the message makes an HBM round trip
// and the map is read and written twice over; here a wave owns 16-pixel fragments and does both contractions on them:
//   * stage one: v_mfma_f32_16x16x32_bf16 over the C / 32 chunks against the compress weights, epilogue acc * scale + shift, ReLU, round to bf16;
//   * stage two reads that result FROM THE ACCUMULATOR REGISTERS: a lane (fj = pixel, fq = k-slot quarter) holds compressed channels 16 i + 4 fq + r of its
//     pixel for every 16-row tile i, so the packed decompress weights put channel 32 c + 16 h + 4 fq + r into K slot 8 fq + 4 h + r of chunk c
//     (v2x_pack_codec; the "chain order" of the halo kernels' chained 1x1, applied to the second layer's columns instead of the first layer's rows, which
//     keeps the MESSAGE in natural channel order).  Tiles 2 c and 2 c + 1 of stage one ARE the B fragment of chunk c: no LDS round trip, no cross-lane
//     exchange, and the message goes to HBM only when the caller asks for it;
//   * the weights stay on chip for the whole launch: in registers as MFMA A fragments when both matrices are <= 32 fragments (every Cc <= 32, and
//     C = 128 with Cc = 64), else in LDS (64 KiB at 256 -> 64 -> 256, 128 KiB at 256 -> 128 -> 256), stored fragment-major so that a fragment is one
//     conflict-free 16-byte read per lane.  One barrier after the LDS fill, none between fragments;
//   * the next fragment's pixels are loaded before the current one is multiplied; M need not be a multiple of 16 (clamped loads, masked stores).
// The same two device functions are the whole arithmetic of v2x_codec_compress and v2x_codec_decompress (the sender's and the receiver's half):
// decompress(compress(x)) is bit-identical to the fused launch, and a pixel's bits depend on nothing but that pixel.
// Roof: HBM, 2 C bytes in and 2 C out per pixel (+ 2 Cc with the message).
#include "common.h"
#include <string.h>

struct CodecArgs {
    const uint16_t *x;     // [M][C] bf16 (fused, compress)
    const uint16_t *w;     // packed fragments: stage one [CT1][KS1][64][8], stage two [CT2][KS2][64][8]  (v2x_pack_codec)
    const float *ss;       // scale1[16 CT1], shift1[16 CT1], scale2[C], shift2[C]
    uint16_t *y;           // [M][C] bf16 (fused, decompress)
    uint16_t *msg;         // [M][Cc] bf16: output of fused (may be null) and compress, input of decompress
    int M, Cc;
};

enum { CODEC_FUSED = 0, CODEC_COMPRESS = 1, CODEC_DECOMPRESS = 2 };

// acc * scale + shift, ReLU, round: one definition for both stages and all three entry points (an explicit fma: the contraction is not left to the compiler)
__device__ __forceinline__ uint32_t codec_epi2(float a0, float a1, float s0, float s1, float t0, float t1) {
    return v2x_relu_bf16x2(pack_bf16x2(__builtin_fmaf(a0, s0, t0), __builtin_fmaf(a1, s1, t1)));
}

template <int C, int CC, int MODE, bool LDSW>
__global__ __launch_bounds__(LDSW ? 512 : 256) void codec_kernel(const CodecArgs a) {
    constexpr int KS1 = C / 32, CT1 = CC >= 16 ? CC / 16 : 1, KS2 = CC >= 32 ? CC / 32 : 1, CT2 = C / 16;
    constexpr bool S1 = MODE != CODEC_DECOMPRESS, S2 = MODE != CODEC_COMPRESS;
    constexpr int F1 = S1 ? CT1 * KS1 : 0, F2 = S2 ? CT2 * KS2 : 0;       // fragments this launch keeps
    constexpr int NT = LDSW ? 512 : 256;
    const int lane = threadIdx.x & 63;
    const int fj = lane & 15, fq = lane >> 4;
    const int wave = (int)((blockIdx.x * (unsigned)NT + threadIdx.x) >> 6);
    const int n_waves = (int)(gridDim.x * (unsigned)(NT / 64));
    const uint16_t *w1 = a.w, *w2 = a.w + (size_t)CT1 * KS1 * 512;

    extern __shared__ uint4 codec_lds[];                            // LDSW: [F1 + F2][64] fragments of 16 bytes per lane
    bf16x8_t A1[LDSW ? 1 : (F1 ? F1 : 1)], A2[LDSW ? 1 : (F2 ? F2 : 1)];
    if constexpr (LDSW) {
        if constexpr (S1)
            for (int e = threadIdx.x; e < F1 * 64; e += NT) codec_lds[e] = reinterpret_cast<const uint4 *>(w1)[e];
        if constexpr (S2)
            for (int e = threadIdx.x; e < F2 * 64; e += NT) codec_lds[F1 * 64 + e] = reinterpret_cast<const uint4 *>(w2)[e];
        __syncthreads();
    } else {
#pragma unroll
        for (int f = 0; f < F1; ++f) A1[f] = *reinterpret_cast<const bf16x8_t *>(w1 + ((size_t)f * 64 + lane) * 8);
#pragma unroll
        for (int f = 0; f < F2; ++f) A2[f] = *reinterpret_cast<const bf16x8_t *>(w2 + ((size_t)f * 64 + lane) * 8);
    }
    const float *sc1 = a.ss, *sf1 = a.ss + 16 * CT1, *sc2 = a.ss + 32 * CT1, *sf2 = a.ss + 32 * CT1 + C;

    const int n_frag = (a.M + 15) >> 4;
    if (wave >= n_frag) return;                                      // (after the barrier)

    // what a fragment needs from memory: its pixels' channels (stages one), or its pixels' message in the stage-two slot order
    constexpr int NB = S1 ? KS1 : KS2;
    bf16x8_t B[NB], Bn[NB];
    auto load = [&](bf16x8_t(&dst)[NB], int frag) {
        int p = frag * 16 + fj;
        p = p < a.M ? p : a.M - 1;                                   // clamped: the lanes behind the end load a valid pixel and store nothing
        if constexpr (S1) {
#pragma unroll
            for (int ks = 0; ks < KS1; ++ks) dst[ks] = *reinterpret_cast<const bf16x8_t *>(a.x + (size_t)p * C + ks * 32 + fq * 8);
        } else {
            const uint16_t *m = a.msg + (size_t)p * CC;
#pragma unroll
            for (int c = 0; c < KS2; ++c) {
                uint2 h[2] = {make_uint2(0u, 0u), make_uint2(0u, 0u)};
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int ch = 32 * c + 16 * hh + 4 * fq;             // channels ch .. ch + 3; the padding beyond Cc reads as zero
                    if constexpr (CC >= 4) {
                        if (ch < CC) h[hh] = *reinterpret_cast<const uint2 *>(m + ch);
                    } else if constexpr (CC == 2) {
                        if (ch == 0) h[hh].x = *reinterpret_cast<const uint32_t *>(m);
                    } else {
                        if (ch == 0) h[hh].x = m[0];
                    }
                }
                dst[c] = __builtin_bit_cast(bf16x8_t, make_uint4(h[0].x, h[0].y, h[1].x, h[1].y));
            }
        }
    };

    load(B, wave);
    for (int f = wave; f < n_frag; f += n_waves) {
        const int fn = f + n_waves;
        load(Bn, fn < n_frag ? fn : f);                              // the next fragment is in flight while this one is multiplied
        const int p = f * 16 + fj;
        const bool live = p < a.M;
        // LDS form: the weight reads must stay INSIDE the loop (they are loop-invariant, and hoisted they would be 128 fragments of registers):
        // their address goes through a value the optimiser cannot see through
        int wl = lane;
        if constexpr (LDSW) asm volatile("" : "+v"(wl));

        bf16x8_t B2[KS2];
        if constexpr (S1) {
            uint32_t mx[CT1], my[CT1];                               // tile i: channels 16 i + 4 fq + {0, 1} and {2, 3}, packed bf16
#pragma unroll
            for (int i = 0; i < CT1; ++i) {
                f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS1; ++ks) {
                    bf16x8_t w;
                    if constexpr (LDSW) w = __builtin_bit_cast(bf16x8_t, codec_lds[(i * KS1 + ks) * 64 + wl]);
                    else w = A1[i * KS1 + ks];
                    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, B[ks], acc, 0, 0, 0);
                }
                const float4 s = *reinterpret_cast<const float4 *>(sc1 + i * 16 + fq * 4);
                const float4 t = *reinterpret_cast<const float4 *>(sf1 + i * 16 + fq * 4);
                mx[i] = codec_epi2(acc[0], acc[1], s.x, s.y, t.x, t.y);
                my[i] = codec_epi2(acc[2], acc[3], s.z, s.w, t.z, t.w);
            }
            if (a.msg && live) {                                     // natural channel order
                uint16_t *m = a.msg + (size_t)p * CC;
                if constexpr (CC >= 32) {
#pragma unroll
                    for (int i = 0; i < CT1; i += 2) v2x_store_pair_x4(m + i * 16 + fq * 4, fq, mx[i], my[i], mx[i + 1], my[i + 1]);
                } else if constexpr (CC >= 4) {
                    if (fq * 4 < CC) *reinterpret_cast<uint2 *>(m + fq * 4) = make_uint2(mx[0], my[0]);
                } else if constexpr (CC == 2) {
                    if (fq == 0) *reinterpret_cast<uint32_t *>(m) = mx[0];
                } else {
                    if (fq == 0) m[0] = (uint16_t)(mx[0] & 0xffffu);
                }
            }
            if constexpr (S2) {
#pragma unroll
                for (int c = 0; c < KS2; ++c) {
                    uint32_t hx = 0u, hy = 0u;                       // Cc <= 16: the upper half of the one chunk is padding
                    if constexpr (CT1 >= 2) {
                        hx = mx[2 * c + 1];
                        hy = my[2 * c + 1];
                    }
                    B2[c] = __builtin_bit_cast(bf16x8_t, make_uint4(mx[2 * c], my[2 * c], hx, hy));
                }
            }
        } else {
#pragma unroll
            for (int c = 0; c < KS2; ++c) B2[c] = B[c];
        }

        if constexpr (S2) {
            uint16_t *yo = a.y + (size_t)p * C;
#pragma unroll
            for (int i = 0; i < CT2; i += 2) {
                uint32_t ox[2], oy[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int c = 0; c < KS2; ++c) {
                        bf16x8_t w;
                        if constexpr (LDSW) w = __builtin_bit_cast(bf16x8_t, codec_lds[(F1 + (i + h) * KS2 + c) * 64 + wl]);
                        else w = A2[(i + h) * KS2 + c];
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, B2[c], acc, 0, 0, 0);
                    }
                    const float4 s = *reinterpret_cast<const float4 *>(sc2 + (i + h) * 16 + fq * 4);
                    const float4 t = *reinterpret_cast<const float4 *>(sf2 + (i + h) * 16 + fq * 4);
                    ox[h] = codec_epi2(acc[0], acc[1], s.x, s.y, t.x, t.y);
                    oy[h] = codec_epi2(acc[2], acc[3], s.z, s.w, t.z, t.w);
                }
                // the exchange runs in every lane (v_permlane16_swap_b32 reads its neighbour row), the store only in the live ones
                const auto rx = __builtin_amdgcn_permlane16_swap(ox[0], ox[1], false, false);
                const auto ry = __builtin_amdgcn_permlane16_swap(oy[0], oy[1], false, false);
                if (live) *reinterpret_cast<uint4 *>(yo + i * 16 + fq * 4 + ((fq & 1) ? 12 : 0)) = make_uint4(rx[0], ry[0], rx[1], ry[1]);
            }
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) B[k] = Bn[k];
    }
}


static inline bool codec_cc_ok(int C, int Cc) { return Cc >= 1 && Cc < C && (Cc & (Cc - 1)) == 0; }

template <int C, int CC, int MODE, bool LDSW>
static int codec_launch(const CodecArgs &a, hipStream_t s) {
    constexpr int KS1 = C / 32, CT1 = CC >= 16 ? CC / 16 : 1, KS2 = CC >= 32 ? CC / 32 : 1, CT2 = C / 16;
    constexpr int F = (MODE != CODEC_DECOMPRESS ? CT1 * KS1 : 0) + (MODE != CODEC_COMPRESS ? CT2 * KS2 : 0);
    constexpr int NT = LDSW ? 512 : 256;
    constexpr int lds = LDSW ? F * 1024 : 0;
    if (lds >= 64 * 1024) {   // (kept beside the helper, which asks for none here: this site reports a refused opt-in by itself)
        static v2x_once_per_device once;
        if (v2x_first_use_on_device(once)) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(codec_kernel<C, CC, MODE, LDSW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (e != hipSuccess) {
                v2x_set_error("v2x_codec: hipFuncSetAttribute(%zu bytes of LDS): %s", (size_t)lds, hipGetErrorString(e));
                return V2X_EIO;
            }
        }
    }
    const int n_frag = (a.M + 15) / 16, wpb = NT / 64;
    int grid = (n_frag + wpb - 1) / wpb;
    // LDS form: one 8-wave workgroup per CU while the weights are > 80 KiB, two below; register form: the register file holds 2 workgroups per CU
    const int cap = v2x_num_cus() * (LDSW ? (lds > 80 * 1024 ? 1 : 2) : 2);
    if (grid > cap) grid = cap;
    return v2x_launch<codec_kernel<C, CC, MODE, LDSW>, 0>("codec_kernel", dim3(grid), dim3(NT), lds, s, a);
}

template <int C, int CC, int MODE>
static int codec_mode(const CodecArgs &a, hipStream_t s) {
    if constexpr (CC >= C) return V2X_EINVAL;
    else {
        constexpr int KS1 = C / 32, CT1 = CC >= 16 ? CC / 16 : 1, KS2 = CC >= 32 ? CC / 32 : 1, CT2 = C / 16;
        // fragments of both matrices: <= 32 live in registers, more in LDS; the split launches keep the fused launch's home for the weights
        // (the arithmetic does not depend on it)
        return codec_launch<C, CC, MODE, (CT1 * KS1 + CT2 * KS2 > 32)>(a, s);
    }
}

template <int C, int MODE>
static int codec_cc(const CodecArgs &a, hipStream_t s) {
    switch (a.Cc) {
        case 1: return codec_mode<C, 1, MODE>(a, s);
        case 2: return codec_mode<C, 2, MODE>(a, s);
        case 4: return codec_mode<C, 4, MODE>(a, s);
        case 8: return codec_mode<C, 8, MODE>(a, s);
        case 16: return codec_mode<C, 16, MODE>(a, s);
        case 32: return codec_mode<C, 32, MODE>(a, s);
        case 64: return codec_mode<C, 64, MODE>(a, s);
        case 128: return codec_mode<C, 128, MODE>(a, s);
        default: return V2X_EINVAL;
    }
}

static int codec_check(const char *who, const void *in, const void *out, long long M, int C, int Cc, const void *w, const void *ss) {
    V2X_REQUIRE(in && out && w && ss, "%s: null pointer", who);
    V2X_REQUIRE(C == 128 || C == 256, "%s: C = %d, the kernel is built for 128 and 256 channels", who, C);
    V2X_REQUIRE(codec_cc_ok(C, Cc), "%s: Cc = %d must be a power of two in [1, C / 2]", who, Cc);
    V2X_REQUIRE(M > 0 && M < (1ll << 31) - 64, "%s: M = %lld outside (0, 2^31 - 64)", who, M);
    V2X_REQUIRE(((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(ss)) & 15) == 0,
                "%s: pointers must be 16-byte aligned", who);
    return V2X_OK;
}

template <int MODE>
static int codec_dispatch(const CodecArgs &a, int C, hipStream_t s) {
    return C == 256 ? codec_cc<256, MODE>(a, s) : codec_cc<128, MODE>(a, s);
}

extern "C" int v2x_codec_1x1(const uint16_t *x, long long M, int C, int Cc, const uint16_t *wpack, const float *sspack, uint16_t *y, uint16_t *msg,
                             v2x_stream_t stream) {
    if (int rc = codec_check("v2x_codec_1x1", x, y, M, C, Cc, wpack, sspack)) return rc;
    V2X_REQUIRE((reinterpret_cast<uintptr_t>(msg) & 15) == 0, "v2x_codec_1x1: msg must be 16-byte aligned");
    const CodecArgs a = {x, wpack, sspack, y, msg, (int)M, Cc};
    return codec_dispatch<CODEC_FUSED>(a, C, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int v2x_codec_compress(const uint16_t *x, long long M, int C, int Cc, const uint16_t *wpack, const float *sspack, uint16_t *msg,
                                  v2x_stream_t stream) {
    if (int rc = codec_check("v2x_codec_compress", x, msg, M, C, Cc, wpack, sspack)) return rc;
    const CodecArgs a = {x, wpack, sspack, nullptr, msg, (int)M, Cc};
    return codec_dispatch<CODEC_COMPRESS>(a, C, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int v2x_codec_decompress(const uint16_t *msg, long long M, int C, int Cc, const uint16_t *wpack, const float *sspack, uint16_t *y,
                                    v2x_stream_t stream) {
    if (int rc = codec_check("v2x_codec_decompress", msg, y, M, C, Cc, wpack, sspack)) return rc;
    const CodecArgs a = {nullptr, wpack, sspack, y, const_cast<uint16_t *>(msg), (int)M, Cc};
    return codec_dispatch<CODEC_DECOMPRESS>(a, C, reinterpret_cast<hipStream_t>(stream));
}

// ---- host packer ------------------------------------------------------------------------------------------------------------------------
static inline uint16_t codec_host_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

extern "C" long long v2x_pack_codec_size(int C, int Cc, long long *ss_floats) {
    if (!((C == 128 || C == 256) && codec_cc_ok(C, Cc))) {
        v2x_set_error("v2x_pack_codec_size: C = %d (128 or 256, what the launches take), Cc = %d (a power of two <= C / 2)", C, Cc);
        return V2X_EINVAL;
    }
    const int ct1 = Cc >= 16 ? Cc / 16 : 1, ks2 = Cc >= 32 ? Cc / 32 : 1;
    if (ss_floats) *ss_floats = 32ll * ct1 + 2ll * C;
    return 512ll * (ct1 * (C / 32) + (C / 16) * ks2);
}

extern "C" int v2x_pack_codec(int C, int Cc, const float *wc, const float *scale_c, const float *shift_c, const float *wd, const float *scale_d,
                              const float *shift_d, uint16_t *dst_w, float *dst_ss) {
    V2X_REQUIRE(wc && scale_c && shift_c && wd && scale_d && shift_d && dst_w && dst_ss, "v2x_pack_codec: null pointer");
    V2X_REQUIRE(C == 128 || C == 256, "v2x_pack_codec: C = %d, the kernel is built for 128 and 256 channels", C);
    V2X_REQUIRE(codec_cc_ok(C, Cc), "v2x_pack_codec: Cc = %d must be a power of two in [1, C / 2]", Cc);
    const int ks1 = C / 32, ct1 = Cc >= 16 ? Cc / 16 : 1, ks2 = Cc >= 32 ? Cc / 32 : 1, ct2 = C / 16;
    uint16_t *w1 = dst_w, *w2 = dst_w + (size_t)ct1 * ks1 * 512;
    for (int i = 0; i < ct1; ++i)                                    // stage one, natural: fragment (i, ks), lane 16 fq + fj, j: Wc[16 i + fj][32 ks + 8 fq + j]
        for (int ks = 0; ks < ks1; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int row = 16 * i + (lane & 15), col = 32 * ks + 8 * (lane >> 4) + j;
                    w1[(((size_t)i * ks1 + ks) * 64 + lane) * 8 + j] = row < Cc ? codec_host_bf16(wc[(size_t)row * C + col]) : (uint16_t)0;
                }
    for (int i = 0; i < ct2; ++i)                                    // stage two, chain slots: fragment (i, c), lane, j = 4 h + r: Wd[16 i + fj][32 c + 16 h + 4 fq + r]
        for (int c = 0; c < ks2; ++c)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int row = 16 * i + (lane & 15), col = 32 * c + 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3);
                    w2[(((size_t)i * ks2 + c) * 64 + lane) * 8 + j] = col < Cc ? codec_host_bf16(wd[(size_t)row * Cc + col]) : (uint16_t)0;
                }
    float *sc1 = dst_ss, *sf1 = dst_ss + 16 * ct1, *sc2 = dst_ss + 32 * ct1, *sf2 = sc2 + C;
    for (int r = 0; r < 16 * ct1; ++r) {                             // the padding rows compute relu(0 * 1 + 0) = 0
        sc1[r] = r < Cc ? scale_c[r] : 1.0f;
        sf1[r] = r < Cc ? shift_c[r] : 0.0f;
    }
    for (int r = 0; r < C; ++r) {
        sc2[r] = scale_d[r];
        sf2[r] = shift_d[r];
    }
    return V2X_OK;
}
