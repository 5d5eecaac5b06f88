// half_hook.cpp -- test hook (compiled by tests/test_f16_rows_abi.py with g++): the host's fp32 -> binary16
// rounding of include/expann/half.h over an array, so that it can be compared with numpy's.  No device.
#include <cstddef>
#include <cstdint>

#include "expann/half.h"

extern "C" void f32_to_f16_bits(const float* in, size_t n, uint16_t* out) {
	for (size_t i = 0; i < n; ++i)
		out[i] = expann::f32_to_f16_bits(in[i]);
}
