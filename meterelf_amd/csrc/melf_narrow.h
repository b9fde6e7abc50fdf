// The narrowing rule of the wide RGB frames (melf_process_wide*, melf_wide_to_bgr): how one sample of 16 or 32 bits becomes the byte
// the reading kernels take.  One statement for host and device: k_narrow_rows (k_narrow.hip) and the host packer (melf_narrow_addr.h:
// pack_item) call the functions below, and tests/wide_narrow_main.cpp runs them over every 16-bit pattern against numpy.
// include/meterelf_hip.h writes the rule out for callers:
//     u16             min(s >> shift, 255)                                  (the rule of melf_process_yuv16)
//     f16, bf16, f32  x = the sample widened to float32 (exact)
//                     t = x * scale[c]     rounded to float32
//                     q = t + offset[c]    rounded to float32: two roundings, never a fused multiply-add
//                     r = rintf(q) (ties to even) or floorf(q);  NaN or r < 0 -> 0,  r > 255 -> 255,  otherwise r
// Nothing here depends on a mode a caller can change: the widening of a 16-bit float is exact (integer arithmetic on its bits on the
// host; widen, below, says what the device does), and with |scale| <= 2^24 (the descriptor's check) a product that is
// denormal in float32 is below 2^-102, so that q is offset[c] -- or, with offset[c] zero, a number that rounds to 0 -- whether
// denormals are flushed or not.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/meterelf_hip.h"

#if defined(__HIPCC__)
#define MELF_NARROW_FN __host__ __device__ __forceinline__
#else
#define MELF_NARROW_FN inline
#endif

namespace melf {
namespace narrow {

MELF_NARROW_FN int sample_bytes(int type) { return type == MELF_WIDE_F32 ? 4 : 2; }

// The rule of one call as kernel and packer take it.  scale / offset by POSITION: of the sample inside a packed pixel (the
// descriptor's B, G, R values mapped through the pixel format; position 3, the 4th sample, is never converted), or of the plane in
// the staged planar frame (0 / 1 / 2 = B / G / R).
struct Rule {
    int32_t type;       // MELF_WIDE_*
    int32_t shift;      // MELF_WIDE_U16: low bits dropped
    int32_t floor_;     // the float types: floorf, not rintf
    int32_t channels;   // samples of a packed pixel, 3 or 4; planar: 1
    float scale[4], offset[4];
};

MELF_NARROW_FN float bits_to_float(uint32_t u)
{
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}

// the float32 of a float16's bits: exact, denormals included (m * 2^-24 is a normal float32)
MELF_NARROW_FN uint32_t f16_to_f32_bits(uint32_t h)
{
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return sign | 0x7f800000u | (m << 13);   // inf, NaN
    if (e != 0u) return sign | ((e + 112u) << 23) | (m << 13);
    if (m == 0u) return sign;
    const uint32_t p = 31u - (uint32_t)__builtin_clz(m);   // the highest set bit, 0 .. 9: m * 2^-24 = 2^(p - 24) * (m / 2^p)
    return sign | ((p + 103u) << 23) | ((m << (23u - p)) & 0x7fffffu);
}

// bits: the sample as loaded, zero-extended.  On the device a float16 goes through the conversion instruction (v_cvt_f32_f16): the
// kernels' code objects keep float16 denormals (float_denorm_mode_16_64 = 3, the compiler's default for HIP kernels), under which it
// is the same exact widening as the integer form -- tests/test_wide_frames.py runs every pattern through the kernel.
template <int TYPE>
MELF_NARROW_FN float widen(uint32_t bits)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (TYPE == MELF_WIDE_F16) {
        const uint16_t b = (uint16_t)bits;
        _Float16 h;
        __builtin_memcpy(&h, &b, 2);
        return (float)h;
    }
#endif
    if (TYPE == MELF_WIDE_F16) return bits_to_float(f16_to_f32_bits(bits));
    if (TYPE == MELF_WIDE_BF16) return bits_to_float(bits << 16);
    return bits_to_float(bits);
}

// x * s, then + o: two float32 roundings.  The library is built with -ffp-contract=off (Makefile); the function says so itself as
// well, for a program that includes this header under other flags: clang, host and device, honours the pragma under its own
// default and under hipcc's (fast-honor-pragmas; only a plain -ffp-contract=fast overrides it, and __fmul_rn / __fadd_rn are plain
// operators there too); for other compilers the product passes through memory between the two operations.
MELF_NARROW_FN float scaled(float x, float s, float o)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float t = x * s;
#if !defined(__clang__) && defined(__GNUC__)
    __asm__ volatile("" : "+m"(t));
#endif
    return t + o;
}

MELF_NARROW_FN uint32_t to_byte(float q, bool floor_)
{
    const float r = floor_ ? floorf(q) : rintf(q);
    if (!(r >= 0.0f)) return 0u;   // NaN, -inf, every negative number
    if (r > 255.0f) return 255u;   // +inf too
    return (uint32_t)(int)r;
}

MELF_NARROW_FN uint32_t narrow_u16(uint32_t s, int shift)
{
    const uint32_t v = s >> shift;
    return v < 255u ? v : 255u;
}

template <int TYPE>
MELF_NARROW_FN uint32_t narrow_sample(uint32_t bits, int shift, float s, float o, bool floor_)
{
    if (TYPE == MELF_WIDE_U16) return narrow_u16(bits, shift);
    return to_byte(scaled(widen<TYPE>(bits), s, o), floor_);
}

// the position of sample j of a packed row (counted from a pixel's first sample) / of every sample of plane `plane`
MELF_NARROW_FN uint32_t position(uint32_t channels, uint32_t plane, uint32_t j) { return channels == 1u ? plane : j % channels; }

// Host: `count` samples from src (aligned to the sample size at most: every load is a memcpy) to count bytes at dst.  Sample i is
// sample j0 + i of its row.  A sample at position 3 is not loaded; its byte is 0.
template <int TYPE>
inline void narrow_samples_t(uint8_t* dst, const uint8_t* src, uint32_t count, uint32_t j0, uint32_t plane, const Rule& r)
{
    constexpr int SS = TYPE == MELF_WIDE_F32 ? 4 : 2;
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t pos = position((uint32_t)r.channels, plane, j0 + i);
        if (pos == 3u) { dst[i] = 0; continue; }
        uint32_t bits = 0;
        memcpy(&bits, src + (size_t)i * SS, SS);   // little-endian samples
        dst[i] = (uint8_t)narrow_sample<TYPE>(bits, r.shift, r.scale[pos], r.offset[pos], r.floor_ != 0);
    }
}
inline void narrow_samples(uint8_t* dst, const uint8_t* src, uint32_t count, uint32_t j0, uint32_t plane, const Rule& r)
{
    switch (r.type) {
    case MELF_WIDE_U16: narrow_samples_t<MELF_WIDE_U16>(dst, src, count, j0, plane, r); break;
    case MELF_WIDE_F16: narrow_samples_t<MELF_WIDE_F16>(dst, src, count, j0, plane, r); break;
    case MELF_WIDE_BF16: narrow_samples_t<MELF_WIDE_BF16>(dst, src, count, j0, plane, r); break;
    default: narrow_samples_t<MELF_WIDE_F32>(dst, src, count, j0, plane, r); break;
    }
}

}  // namespace narrow
}  // namespace melf
