// k_lora.hip -- the LoRA merge (sdmi_lora_set_scale): W = W0 + sum_t coef_t (P_t Q_t) on one fp32 weight tensor seen as a
// row-major matrix [R][Cc] in the reference's layout.  No reference counterpart: the reference runs the base checkpoint only.
//
// The kernel is bound by the master's bytes (one 16-byte read and one 16-byte write per four elements); the rank-r products are vector FMAs on
// factors staged through LDS, JC = 16 rank columns at a time.  A 256-thread workgroup owns a 32 x 128 tile: thread (tx, ty) holds columns
// 4 tx .. 4 tx + 3 of rows ty, ty + 8, ty + 16, ty + 24, so a wave reads two 512-byte row segments per row step and the LDS reads are one
// conflict-free 16-byte read of Q per rank column plus broadcast reads of P.  LDS: (16 x 33 + 16 x 132) x 4 = 10.3 KB, 32 + 32 live
// accumulator registers -- occupancy is not what limits a kernel that streams each byte once.  The factors are addressed with element
// strides, so a Linear target (master [in][out], delta[i][o] = sum_j up[o][j] down[j][i]) reads up and down as stored; which index runs
// fastest while staging follows the unit stride.  No atomics, a fixed summation order: bit-identical run to run.
//
// Order of operations (the rounding bound of tests/test_lora_gpu.py rests on it): per term d = fma(P(r, j), Q(j, c), d) for j = 0 .. rank - 1
// from d = 0, then w = fma(coef, d, w), terms in the order given, w starting at W0.  Rank columns past `rank` are staged as zeros (d + 0 * 0).
//
// Factor dtype (a kohya .safetensors file holds its factors as F16, mostly): the two staging loops widen a 16-bit element exactly, on its bit pattern
// (k_widen.hpp, the conversions of k_unpack.hip), while they fill Ps / Qs; the FMA loop never sees the storage type.  The type is a template parameter, not a
// branch: lora_merge_kernel, the F32 instance, is the kernel as it was -- 118 VGPRs, 10560 bytes of LDS, no scratch; tests/test_lora_file_cpu.py holds the
// figures -- and the five instances a file brings are lora_factor_merge_kernel<DT, HADA>, all stamped from one body (k_lora_tile.inc), so every
// launch that sdmi_lora_add feeds produces the bits it always did.  16-bit elements are read one at a time: along the unit-stride index consecutive lanes read
// consecutive 2-byte elements (whole contiguous segments per wave, half the bytes of fp32), and a row of odd length may start at any 2-byte offset.
//
// LoHa terms (HADA = true; LoraTerm::kind 1): W += coef (P Q) o (P2 Q2).  Both products share the rank chunk loop and are staged side by side, so LDS doubles to
// 2 x 10560 = 21120 bytes and the accumulators to 64 registers (120 VGPRs in the build, no scratch): still several workgroups per CU, and occupancy is no concern
// for a kernel that streams the master once.  Order of operations (the bound of tests/lora_file_ref.py rests on it): d1 and d2 are each the FMA chain above over
// j = 0 .. rank - 1 from 0, h = d1 * d2 rounded once, w = fma(coef, h, w).  A launch holds terms of one dtype and one kind; the engine cuts a mixed list into
// launches that continue in place (as it does after kLoraMaxTerms terms), which changes no element's order of operations.  LoraMerge is a by-value kernel
// argument: 32 + 8 x 112 = 928 bytes of the 4 KB segment (static_assert in kernels.hpp).
#include "k_widen.hpp"
#include "kernels.hpp"

namespace sdmi {

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr int kTR = 32, kTC = 128, kJC = 16;

// element i of a factor stored as DT (0 F32, 1 F16, 2 BF16): 16-bit elements are read one by one -- consecutive lanes read consecutive 2-byte elements
// along the unit-stride index, so a wave's request is still whole contiguous segments, and no row has to start 4-byte aligned
template <int DT>
__device__ __forceinline__ float factor_at(const void* f, long long i) {
    if (DT == 0) return reinterpret_cast<const float*>(f)[i];
    return half_bits_to_f32<DT>(reinterpret_cast<const unsigned short*>(f)[i]);
}
}  // namespace

// F32 factors, plain terms: the kernel every sdmi_lora_add launch runs, under the name and with the resources it always had
__global__ __launch_bounds__(256) void lora_merge_kernel(LoraMerge m) {
    constexpr int DT = 0;
    constexpr bool HADA = false;
#include "k_lora_tile.inc"
}

// the instances a file brings: 16-bit factors, LoHa terms
template <int DT, bool HADA>
__global__ __launch_bounds__(256) void lora_factor_merge_kernel(LoraMerge m) {
#include "k_lora_tile.inc"
}

hipError_t launch_lora_merge(const LoraMerge& m, hipStream_t s) {
    if (!m.W0 || !m.W || m.R <= 0 || m.Cc <= 0 || m.n_terms < 0 || m.n_terms > kLoraMaxTerms) return hipErrorInvalidValue;
    if ((m.Cc & 3) == 0 && ((reinterpret_cast<uintptr_t>(m.W0) | reinterpret_cast<uintptr_t>(m.W)) & 15)) return hipErrorInvalidValue;
    const int dtype = m.n_terms ? m.t[0].dtype : 0, kind = m.n_terms ? m.t[0].kind : 0;
    if (dtype < 0 || dtype > 2 || kind < 0 || kind > 1) return hipErrorInvalidValue;
    for (int t = 0; t < m.n_terms; ++t) {
        const LoraTerm& lt = m.t[t];
        if (!lt.P || !lt.Q || lt.rank < 1 || lt.dtype != dtype || lt.kind != kind) return hipErrorInvalidValue;
        if (kind == 1 && (!lt.P2 || !lt.Q2)) return hipErrorInvalidValue;
        const uintptr_t all = reinterpret_cast<uintptr_t>(lt.P) | reinterpret_cast<uintptr_t>(lt.Q) | reinterpret_cast<uintptr_t>(lt.P2) | reinterpret_cast<uintptr_t>(lt.Q2);
        if (all & (dtype == 0 ? 3u : 1u)) return hipErrorInvalidValue;   // an element is read with one aligned load
    }
    const long long gy = ((long long)m.R + kTR - 1) / kTR;
    if (gy > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((m.Cc + kTC - 1) / kTC), (unsigned)gy);
    switch (2 * dtype + kind) {
        case 0: hipLaunchKernelGGL(lora_merge_kernel, grid, dim3(256), 0, s, m); break;
        case 1: hipLaunchKernelGGL((lora_factor_merge_kernel<0, true>), grid, dim3(256), 0, s, m); break;
        case 2: hipLaunchKernelGGL((lora_factor_merge_kernel<1, false>), grid, dim3(256), 0, s, m); break;
        case 3: hipLaunchKernelGGL((lora_factor_merge_kernel<1, true>), grid, dim3(256), 0, s, m); break;
        case 4: hipLaunchKernelGGL((lora_factor_merge_kernel<2, false>), grid, dim3(256), 0, s, m); break;
        default: hipLaunchKernelGGL((lora_factor_merge_kernel<2, true>), grid, dim3(256), 0, s, m); break;
    }
    return hipGetLastError();
}

}  // namespace sdmi
