// philox.h -- the counter-based noise source of cine_noise_add (include/cine_hip.h states the definition; this is its one
// implementation).  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), the map
// from two 32-bit words to a complex normal with E|z|^2 = 1, and the fmaf chain of the coloured noise.
//
// Compiles for the device (hipcc) and for the host (g++: tests/host/philox_host_check.cpp checks the known-answer vectors, the
// 64-bit point counter and the uniforms without a GPU).  A value depends on (seed, replica, point, coil) only.
#pragma once

#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#else
#include <cmath>
#endif

#ifndef CINE_HD
#if defined(__HIPCC__)
#define CINE_HD __host__ __device__ __forceinline__
#else
#define CINE_HD inline
#endif
#endif

namespace cine {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;      // multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;      // Weyl increments of the key

struct Philox4 { uint32_t x[4]; };
struct PhiloxNormal { float re, im; };

// ten rounds of (c0,c1,c2,c3) -> (hi(M1 c2)^c1^k0, lo(M1 c2), hi(M0 c0)^c3^k1, lo(M0 c0)), the key bumped after every round
CINE_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
    Philox4 o;
    o.x[0] = c0; o.x[1] = c1; o.x[2] = c2; o.x[3] = c3;
    return o;
}

// the four words of k-space point p, coil pair j: key = the seed's two halves, counter = (p lo, p hi, replica, j)
CINE_HD Philox4 philox_point(long seed, long replica, uint64_t p, int pair) {
    const uint64_t s = (uint64_t)seed;
    return philox4x32_10((uint32_t)p, (uint32_t)(p >> 32), (uint32_t)replica, (uint32_t)pair, (uint32_t)s, (uint32_t)(s >> 32));
}

// u1 in [2^-24, 1 - 2^-24], u2 in [0, 1): every step is exact in float32
CINE_HD float philox_u1(uint32_t a) { return ((float)(a >> 9) + 0.5f) * 1.1920928955078125e-07f; }      // 2^-23
CINE_HD float philox_u2(uint32_t b) { return (float)(b >> 8) * 5.9604644775390625e-08f; }               // 2^-24

// z = sqrt(-log u1) (cos 2 pi u2 + i sin 2 pi u2): E|z|^2 = E[-log u1] = 1
CINE_HD PhiloxNormal philox_normal(uint32_t a, uint32_t b) {
    const float r = sqrtf(-logf(philox_u1(a)));
    const float ang = 2.0f * philox_u2(b);
    float s, c;
#if defined(__HIP_DEVICE_COMPILE__)
    sincospif(ang, &s, &c);
#else
    s = (float)std::sin(3.14159265358979323846 * (double)ang);       // the host has no sincospif: the double functions, rounded
    c = (float)std::cos(3.14159265358979323846 * (double)ang);
#endif
    PhiloxNormal z;
    z.re = r * c; z.im = r * s;
    return z;
}

// the normal of one coil of point p: coil 2j takes (x0, x1), coil 2j + 1 takes (x2, x3)
CINE_HD PhiloxNormal philox_coil_normal(long seed, long replica, uint64_t p, int coil) {
    const Philox4 v = philox_point(seed, replica, p, coil >> 1);
    return (coil & 1) ? philox_normal(v.x[2], v.x[3]) : philox_normal(v.x[0], v.x[1]);
}

// acc += l * z, one step of eta_i = sum_{k <= i} L[i, k] z_k (ascending k): four fmaf in this order
CINE_HD void philox_cfma(float& acc_re, float& acc_im, float l_re, float l_im, PhiloxNormal z) {
    acc_re = fmaf(l_re, z.re, acc_re);
    acc_re = fmaf(-l_im, z.im, acc_re);
    acc_im = fmaf(l_re, z.im, acc_im);
    acc_im = fmaf(l_im, z.re, acc_im);
}

}  // namespace cine
