// Host check of csrc/philox.h: the Random123 known-answer vectors of philox4x32-10, then a dump of what the header draws for a
// run of k-space points -- per (point, coil) the two words, the two uniforms and the normal -- which tests/test_noise_cpu.py
// compares with tests/noise_reference.py.
// Build: g++ -O2 -std=c++17 -I<csrc> philox_host_check.cpp -o philox_host_check
// Run:   philox_host_check <seed> <replica> <point0> <points> <coils> <out file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "philox.h"
using namespace cine;

struct Kat { uint32_t c[4], k[2], want[4]; };
static const Kat kKat[3] = {
    {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
    {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
    {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
};

struct Rec { uint32_t a, b; float u1, u2, re, im; };

int main(int argc, char** argv) {
    for (const Kat& t : kKat) {
        const Philox4 o = philox4x32_10(t.c[0], t.c[1], t.c[2], t.c[3], t.k[0], t.k[1]);
        if (std::memcmp(o.x, t.want, sizeof t.want) != 0) {
            std::printf("known-answer vector FAILED: %08x %08x %08x %08x\n", o.x[0], o.x[1], o.x[2], o.x[3]);
            return 1;
        }
    }
    std::printf("known-answer vectors ok\n");
    if (argc != 7) return 0;
    const long seed = std::strtol(argv[1], nullptr, 0), replica = std::strtol(argv[2], nullptr, 0);
    const uint64_t point0 = std::strtoull(argv[3], nullptr, 0);
    const long n = std::strtol(argv[4], nullptr, 0);
    const int c = std::atoi(argv[5]);
    std::FILE* f = std::fopen(argv[6], "wb");
    if (!f || n < 1 || c < 1) return 2;
    for (long i = 0; i < n; ++i)
        for (int coil = 0; coil < c; ++coil) {
            const Philox4 v = philox_point(seed, replica, point0 + (uint64_t)i, coil >> 1);
            Rec r;
            r.a = v.x[(coil & 1) * 2]; r.b = v.x[(coil & 1) * 2 + 1];
            r.u1 = philox_u1(r.a); r.u2 = philox_u2(r.b);
            const PhiloxNormal z = philox_coil_normal(seed, replica, point0 + (uint64_t)i, coil);
            r.re = z.re; r.im = z.im;
            std::fwrite(&r, sizeof r, 1, f);
        }
    std::fclose(f);
    std::printf("wrote %ld points x %d coils\n", n, c);
    return 0;
}
