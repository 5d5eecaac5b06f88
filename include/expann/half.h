// half.h -- fp32 -> IEEE binary16 as a bit-level function, for hosts whose compiler has no _Float16.
//
// expann::f32_to_f16_bits rounds to nearest, ties to even -- what a hardware convert and
// numpy's astype(float16) do: overflow (|x| >= 65520) gives +-inf, values below the smallest
// normal half (2^-14) give subnormals, |x| <= 2^-25 gives +-0, a NaN stays a NaN (quiet, sign and
// the top mantissa bits kept).  The rows of an EXPANN_DTYPE_F16 index are these 16-bit patterns.
#pragma once

#include <cstdint>
#include <cstring>

namespace expann {

inline uint16_t f32_to_f16_bits(float f) {
	uint32_t x;
	std::memcpy(&x, &f, sizeof(x));
	const uint16_t sign = uint16_t((x >> 16) & 0x8000u);
	const uint32_t ax = x & 0x7fffffffu;
	if (ax > 0x7f800000u)  // NaN
		return uint16_t(sign | 0x7e00u | ((ax >> 13) & 0x01ffu));
	if (ax >= 0x477ff000u)  // inf, and everything from 65520 = (65504 + 65536) / 2 up: the tie goes to the even 2^16
		return uint16_t(sign | 0x7c00u);
	if (ax >= 0x38800000u) {  // normal half: rebias the exponent (127 - 15), round the 13 dropped bits
		const uint32_t v = ax - 0x38000000u;
		return uint16_t(sign | ((v + 0x0fffu + ((v >> 13) & 1u)) >> 13));  // (a carry into the exponent is the right answer)
	}
	if (ax < 0x33000000u)  // below 2^-25: nearer to zero than to the smallest subnormal 2^-24
		return sign;
	// subnormal half: the value is m * 2^(e - 150); in units of 2^-24 that is m >> (126 - e)
	const uint32_t e = ax >> 23;  // 102 .. 112
	const uint32_t m = (ax & 0x007fffffu) | 0x00800000u;
	const uint32_t shift = 126u - e;  // 14 .. 24
	uint32_t q = m >> shift;
	const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
	if (rem > half || (rem == half && (q & 1u)))
		++q;  // (up to 0x400: the smallest normal half)
	return uint16_t(sign | q);
}

// binary16 bits -> fp32, exact (subnormals included; inf and NaN map to inf and NaN)
inline float f16_bits_to_f32(uint16_t h) {
	const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x03ffu;
	uint32_t x;
	if (e == 0x1fu) {
		x = sign | 0x7f800000u | (m << 13);
	} else if (e != 0) {
		x = sign | ((e + 112u) << 23) | (m << 13);
	} else if (m == 0) {
		x = sign;
	} else {  // subnormal half m * 2^-24: normalise
		uint32_t mm = m, ee = 113u;
		while (!(mm & 0x0400u)) {
			mm <<= 1;
			--ee;
		}
		x = sign | (ee << 23) | ((mm & 0x03ffu) << 13);
	}
	float f;
	std::memcpy(&f, &x, sizeof(f));
	return f;
}

}  // namespace expann
