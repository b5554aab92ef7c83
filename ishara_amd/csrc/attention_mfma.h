// What the MFMA attention kernels share: attention_mfma.hip (forward) and attention_bwd_mfma.hip (backward).
#pragma once
#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

#define AF_KC 64     // keys per LDS chunk
#define AF_QB 128    // queries per workgroup
#define AF_VLD 72    // V^T tile row stride (64 keys + 8 pad): 144-B rows make the 8-byte fragment reads conflict-free
#define AF_PAD 8     // row-major [64][DH] tiles get DH+8 columns (80-B / 144-B rows): conflict-free 16-byte fragment reads

DEVI uint32_t pk2(float lo, float hi) {      // ONE v_cvt_pk_bf16_f32 (element-wise casts compile to two of them and a v_perm_b32)
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const f32x2 v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// keepbits |= the four keep flags at bit positions sh .. sh+3 (sh is a compile-time constant after unrolling)
DEVI void constexpr_shift_or(uint32_t& bits, bool k0, bool k1, bool k2, bool k3, int sh) {
    bits |= (k0 ? (1u << sh) : 0u) | (k1 ? (2u << sh) : 0u) | (k2 ? (4u << sh) : 0u) | (k3 ? (8u << sh) : 0u);
}

// XCD-aware workgroup -> (head bh, block xb) mapping.  Workgroups are dealt round-robin to the 8 XCDs (id % 8), each with
// its own L2; the nxb query (key) blocks of one (batch, head) all stream the SAME K/V (Q/dO) rows, so they are given ids
// with the same residue mod 8 and consecutive positions on that XCD: the streamed operand is read from HBM once per head
// instead of once per block.  Grid = nxb * BH workgroups, 1-D.
DEVI void attn_block_of(int nxb, int BH, int& bh, int& xb) {
    const int id = blockIdx.x;
    if ((BH & 7) == 0) { const int xcd = id & 7, j = id >> 3; bh = (j / nxb) * 8 + xcd; xb = j % nxb; }
    else { bh = id / nxb; xb = id % nxb; }
}

// DM: dropout mode, compile-time so that no per-score uniform branch is left: 0 none, 1 counter hash, 2 counter hash in the
// forward + keep bits cached in `maskbits` for the two backward kernels
template <typename E> struct af_vec;
template <> struct af_vec<bf16> { typedef bf16x8 v8; typedef bf16x4 v4; };
template <> struct af_vec<f16> { typedef f16x8 v8; typedef __attribute__((ext_vector_type(4))) _Float16 v4; };
DEVI f32x4 af_mfma(bf16x8 a, bf16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }
DEVI f32x4 af_mfma(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
template <typename E> DEVI uint32_t pk2e(float lo, float hi);
template <> DEVI uint32_t pk2e<bf16>(float lo, float hi) { return pk2(lo, hi); }
template <> DEVI uint32_t pk2e<f16>(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    f16x2 t; t[0] = (f16)lo; t[1] = (f16)hi;
    return __builtin_bit_cast(uint32_t, t);
}

// Host: a route's dm (0 / 1 / 2) as the template argument DM — fn(att_int<DM>{}) — and the workgroups of the tiled kernels
template <typename F> static int att_by_dm(int dm, F fn) { return dm == 0 ? fn(att_int<0>{}) : (dm == 1 ? fn(att_int<1>{}) : fn(att_int<2>{})); }
static inline dim3 af_grid(int B, int H, int T) { return dim3(((T + AF_QB - 1) / AF_QB) * B * H); }
