// k_widen.hpp -- the exact widening of a 16-bit float's bit pattern to fp32, shared by the checkpoint unpack kernels (k_unpack.hip) and the LoRA merge
// (k_lora.hip), so that a factor a file holds as F16 / BF16 reaches the FMA chain as the value the host's widening gives, bit for bit.
//   BF16  bits << 16;
//   F16   sign, exponent re-biased by 112, mantissa << 13; a subnormal is normalised with a count of leading zeros; inf / NaN keep their payload.
#pragma once
#include <hip/hip_runtime.h>

namespace sdmi {

__device__ __forceinline__ float f16_bits_to_f32(unsigned h) {
    const unsigned sign = (h & 0x8000u) << 16;
    const unsigned ex = (h >> 10) & 31u;
    unsigned man = h & 0x3ffu;
    unsigned bits;
    if (ex == 0) {
        if (man == 0) {
            bits = sign;
        } else {   // subnormal: man 2^-24 = 1.f 2^(-14 - s), s = the shift that brings the leading one to bit 10
            const unsigned s = (unsigned)__clz((int)man) - 21u;
            man = (man << s) & 0x3ffu;
            bits = sign | ((113u - s) << 23) | (man << 13);
        }
    } else if (ex == 31) {
        bits = sign | 0x7f800000u | (man << 13);
    } else {
        bits = sign | ((ex + 112u) << 23) | (man << 13);
    }
    return __uint_as_float(bits);
}

// DT: 0 F32, 1 F16, 2 BF16
template <int DT>
__device__ __forceinline__ float half_bits_to_f32(unsigned h) {
    return DT == 1 ? f16_bits_to_f32(h) : __uint_as_float(h << 16);
}

}  // namespace sdmi
