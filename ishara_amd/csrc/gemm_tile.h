// Device helpers shared by the NT and TN tile kernels (gemm_nt.hip, gemm_tn.hip): MFMA tile configuration, operand transforms,
// chunk loads / packs, the LDS swizzle, the fragment readers and the NT operand stager.  Private to the GEMM sources.
#pragma once
#include <type_traits>
#include "kernels.h"

typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

template <typename TM> struct MmaCfg;
template <> struct MmaCfg<bf16>  { static constexpr int EPC = 8; static constexpr int BK = 64; };
template <> struct MmaCfg<f16>   { static constexpr int EPC = 8; static constexpr int BK = 64; };
template <> struct MmaCfg<float> { static constexpr int EPC = 4; static constexpr int BK = 32; };

// ---------------------------------------------------------------------------------
// operand transforms
// ---------------------------------------------------------------------------------
template <int N>
DEVI void apply_op(int op, float (&v)[N], int row, int col, const OpArgs& a) {
    switch (op) {
        case OP_SWISH:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = swishf_(v[e]);
            break;
        case OP_COLAFFINE:
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = v[e] * a.c1[col + e] + a.c0[col + e];
            break;
        case OP_ROWSCALE: {
            const float s = a.rs[row / a.T];
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] *= s;
        } break;
        case OP_DROPMASK:
            if (a.drop.thr) {
                const uint32_t rk = rng_row_key(a.drop.key, (uint32_t)row);
#pragma unroll
                for (int e = 0; e < N; ++e) v[e] = rng_keep(rk, (uint32_t)(col + e), a.drop.thr) ? v[e] * a.drop.scale : 0.f;
            }
            break;
        default: break;
    }
}

// load N (4 or 8) consecutive elements of row `row` starting at column `col`, zero filled outside
// [rows x cols].  Row strides are multiples of 16 bytes (launchers enforce cols % 4 == 0 for f32,
// cols % 8 == 0 for bf16), so a chunk is made of whole 16-byte pieces: no element-granular tail.
template <typename T, int N>
DEVI void load_row_chunk(const T* __restrict__ base, int ld, int rows, int cols, int row, int col,
                         bool /*vec_ok*/, float (&v)[N]) {
#pragma unroll
    for (int e = 0; e < N; ++e) v[e] = 0.f;
    if (row >= rows) return;
    const T* p = base + (size_t)row * ld + col;
    if constexpr (is_16b_t<T>::value) {
        if (col + N <= cols) {
            if constexpr (N == 8) load8(p, v);
            else load4g(p, v);
        }
    } else {
#pragma unroll
        for (int h = 0; h < N / 4; ++h) {
            if (col + 4 * h + 4 <= cols) {
                const float4 x = *reinterpret_cast<const float4*>(p + 4 * h);
                v[4 * h] = x.x; v[4 * h + 1] = x.y; v[4 * h + 2] = x.z; v[4 * h + 3] = x.w;
            }
        }
    }
}

DEVI uint32_t pack_bf16x2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
    bf16x2 t; t[0] = (bf16)lo; t[1] = (bf16)hi;
    return __builtin_bit_cast(uint32_t, t);
}
DEVI uint32_t pack_f16x2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) _Float16 f16x2;
    f16x2 t; t[0] = (f16)lo; t[1] = (f16)hi;
    return __builtin_bit_cast(uint32_t, t);
}
template <typename TM, int N> DEVI u32x4 pack_chunk(const float (&v)[N]) {
    u32x4 r;
    if constexpr (std::is_same<TM, f16>::value) {
        r.x = pack_f16x2(v[0], v[1]); r.y = pack_f16x2(v[2], v[3]);
        r.z = pack_f16x2(v[4], v[5]); r.w = pack_f16x2(v[6], v[7]);
    } else if constexpr (is_bf16_t<TM>::value) {
        r.x = pack_bf16x2(v[0], v[1]); r.y = pack_bf16x2(v[2], v[3]);
        r.z = pack_bf16x2(v[4], v[5]); r.w = pack_bf16x2(v[6], v[7]);
    } else {
        r.x = __float_as_uint(v[0]); r.y = __float_as_uint(v[1]);
        r.z = __float_as_uint(v[2]); r.w = __float_as_uint(v[3]);
    }
    return r;
}

// ---------------------------------------------------------------------------------
// MFMA over one LDS tile pair.  ldsA/ldsB: [128 rows][128 bytes], 16-byte slots XOR
// swizzled by SWZ(row).  acc[i][j] = 16x16 tile (rows wr*64+16i.., cols wc*64+16j..).
// ---------------------------------------------------------------------------------
template <int SW> DEVI int swz(int row) { return SW == 0 ? (row & 7) : ((row ^ (row >> 3)) & 7); }

template <typename TM, int SW>
DEVI void mma_tile(const char* ldsA, const char* ldsB, int wr, int wc, int lane, f32x4 (&acc)[4][4]) {
    const int r = lane & 15, g = lane >> 4;
    if constexpr (std::is_same<TM, f16>::value) {      // same tile layout as bf16, the f16 MFMA
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            f16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wr * 64 + 16 * i + r;
                a[i] = *reinterpret_cast<const f16x8*>(ldsA + row * 128 + (((4 * s + g) ^ swz<SW>(row)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wc * 64 + 16 * j + r;
                b[j] = *reinterpret_cast<const f16x8*>(ldsB + row * 128 + (((4 * s + g) ^ swz<SW>(row)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    } else if constexpr (is_bf16_t<TM>::value) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            bf16x8 a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wr * 64 + 16 * i + r;
                a[i] = *reinterpret_cast<const bf16x8*>(ldsA + row * 128 + (((4 * s + g) ^ swz<SW>(row)) << 4));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wc * 64 + 16 * j + r;
                b[j] = *reinterpret_cast<const bf16x8*>(ldsB + row * 128 + (((4 * s + g) ^ swz<SW>(row)) << 4));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = wr * 64 + 16 * i + r;
                a[i] = *reinterpret_cast<const float*>(ldsA + row * 128 + ((s ^ swz<SW>(row)) << 4) + g * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = wc * 64 + 16 * j + r;
                b[j] = *reinterpret_cast<const float*>(ldsB + row * 128 + ((s ^ swz<SW>(row)) << 4) + g * 4);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
}

#include "gemm_epi.h"

// stage one K tile of A (transformed) and Bt into registers: 4 x 16-byte chunks each per thread
template <typename TA, typename TM, int OP>
DEVI void nt_gload(const TA* __restrict__ A, const TM* __restrict__ Bt, int M, int K, int ldb, bool a_vec_ok,
                   int m0, int n0, int kt, int tid, const OpArgs& oa, u32x4 (&ra)[4], u32x4 (&rb)[4]) {
    constexpr int EPC = MmaCfg<TM>::EPC, BK = MmaCfg<TM>::BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i, row = c >> 3, slot = c & 7;
        const int k = kt * BK + slot * EPC;
        float v[EPC];
        load_row_chunk<TA, EPC>(A, K, M, K, m0 + row, k, a_vec_ok, v);
        if (OP != OP_NONE) {
            apply_op<EPC>(OP, v, m0 + row, k, oa);
            if (m0 + row >= M) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[e] = 0.f;
            } else if (k + EPC > K) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) if (k + e >= K) v[e] = 0.f;
            }
        }
        ra[i] = pack_chunk<TM, EPC>(v);
        rb[i] = *reinterpret_cast<const u32x4*>(Bt + (size_t)(n0 + row) * ldb + k);
    }
}
DEVI void nt_lstore(char* sa, int tid, const u32x4 (&ra)[4], const u32x4 (&rb)[4]) {
    char* sb = sa + 16384;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tid + 256 * i, row = c >> 3, slot = c & 7;
        const int off = row * 128 + ((slot ^ (row & 7)) << 4);
        *reinterpret_cast<u32x4*>(sa + off) = ra[i];
        *reinterpret_cast<u32x4*>(sb + off) = rb[i];
    }
}

