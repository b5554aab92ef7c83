// Depthwise conv over time (causal / same padding, fused Swish / GLU input op, fused BatchNorm + GAP statistics): the forward kernels
// (64 x 128 LDS tile, register window, 8-channel register window, streaming LDS ring), the choice among them and among the backward
// kernels (dwconv_fwd_route / dwconv_bwd_route: the one place that decides), and the three launchers.  The tile and register-window
// kernels also run the data gradient of the two-pass backward, which is why the backward launchers live here; the one-pass backward
// kernel and the weight-gradient kernels are in dwconv_bwd.hip.  Activations are [B*T, C] row-major (channel fastest), read and
// written as 16-byte (8 x bf16) or 2 x 16-byte (8 x f32) chunks per lane; all arithmetic is fp32.
#include "kernels.h"

// =====================================================================================
// Depthwise conv over time.  One workgroup = 64 output steps x 128 channels of one sample.
// The input tile (+ k-1 halo) is transformed once (Swish / GLU) and staged in LDS as fp32;
// each thread slides an 8-step register window over its 4 channels.
//   OUT_NONE  : y = conv (+bias), optional per-sample sum / sum-of-squares (BN stats, GAP)
//   OUT_DSWISH: y = conv * swish'(aux)                 (backward through a Swish input op)
//   OUT_DGLU  : y[:, :C] = conv*sig(a2) ; y[:, C:] = conv*a1*sig(a2)*(1-sig(a2))   (aux has 2C)
// `flip` indexes the taps in reverse (backward data pass).
// =====================================================================================
enum : int { OUT_NONE = 0, OUT_DSWISH = 1, OUT_DGLU = 2 };
#define DW_TT 64      // DW_CT (128 channels), DW_MAXK: kernels.h

// KC: compile-time tap count (11: the tap loop is fully unrolled, so the 8-row register window slides by renaming
// instead of 28 v_mov per tap and the tap weights are loaded ahead of use); 0: run-time k
template <typename T, int KC, int KM>      // KC: unrolled tap count (0 = runtime k); KM: largest k this instantiation takes (sizes the LDS tile: 37 / 40 / 48 KB)
__global__ __launch_bounds__(256) void dwconv_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     T* __restrict__ y, const T* __restrict__ aux,
                                                     float* __restrict__ ssum, float* __restrict__ ssq,
                                                     int B, int Tn, int C, int k, int padl, int inop, int outop, int flip, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float tile[(DW_TT + KM - 1) * DW_CT];
    const int tid = threadIdx.x;
    const int t0 = blockIdx.x * DW_TT, c0 = blockIdx.y * DW_CT, b = blockIdx.z;
    const int Cin = (inop == DWIN_GLU) ? 2 * C : C;
    const int rows = DW_TT + k - 1;
    // ---- stage: thread -> chunk (tid&15) of 8 channels, rows (tid>>4) + 16*it.  All global loads of the
    // tile are issued before the first use (rows <= 94 -> at most 6 row groups per thread).
    {
        const int ch = c0 + (tid & 15) * 8;
        constexpr int NIT = (DW_TT + KM - 1 + 15) / 16;
        float v[NIT][8], gl[NIT][8];
        bool ok[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int r = (tid >> 4) + 16 * it;
            const int tin = t0 - padl + r;
            ok[it] = r < rows && tin >= 0 && tin < Tn && ch < C;
            if (ok[it]) {
                const T* p = x + ((size_t)b * Tn + tin) * Cin + ch;
                load8(p, v[it]);
                if (inop == DWIN_GLU) load8(p + C, gl[it]);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int r = (tid >> 4) + 16 * it;
            if (r < rows) {
                if (ok[it]) {
                    if (inop == DWIN_SWISH) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[it][e] = swishf_(v[it][e]);
                    } else if (inop == DWIN_GLU) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[it][e] *= sigmoidf_(gl[it][e]);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[it][e] = 0.f;
                }
                float* dst = tile + r * DW_CT + (tid & 15) * 8;
                *reinterpret_cast<float4*>(dst) = make_float4(v[it][0], v[it][1], v[it][2], v[it][3]);
                *reinterpret_cast<float4*>(dst + 4) = make_float4(v[it][4], v[it][5], v[it][6], v[it][7]);
            }
        }
    }
    __syncthreads();
    // ---- compute: thread -> 4 channels (cl) x 8 consecutive steps (tl)
    const int cl = tid & 31, tl = tid >> 5;
    const int ch = c0 + cl * 4;
    const bool cact = ch < C;
    float acc[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = 0.f;
    if (cact) {
        float4 win[8];
        const float* tp = tile + (tl * 8) * DW_CT + cl * 4;
#pragma unroll
        for (int r = 0; r < 7; ++r) win[r + 1] = *reinterpret_cast<const float4*>(tp + r * DW_CT);
        // invariant at tap j: win[1..7] = tile rows tl*8 + j + (0..6); each tap shifts and loads one row
        auto tap = [&](int j) {
#pragma unroll
            for (int r = 0; r < 7; ++r) win[r] = win[r + 1];
            win[7] = *reinterpret_cast<const float4*>(tp + (j + 7) * DW_CT);
            const float4 wj = *reinterpret_cast<const float4*>(w + (size_t)(flip ? (k - 1 - j) : j) * C + ch);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                acc[r][0] += wj.x * win[r].x; acc[r][1] += wj.y * win[r].y;
                acc[r][2] += wj.z * win[r].z; acc[r][3] += wj.w * win[r].w;
            }
        };
        if constexpr (KC > 0) {
#pragma unroll
            for (int j = 0; j < KC; ++j) tap(j);
        } else {
            for (int j = 0; j < k; ++j) tap(j);
        }
    }
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    if (cact) {
        float bv[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
#pragma unroll
            for (int e = 0; e < 4; ++e) bv[e] = bias[ch + e];
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int t = t0 + tl * 8 + r;
            if (t < Tn) {
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) { o[e] = acc[r][e] + bv[e]; s1[e] += o[e]; s2[e] += o[e] * o[e]; }
                const size_t row = (size_t)b * Tn + t;
                if (outop == OUT_NONE) {
                    store4(y + row * C + ch, o);
                } else if (outop == OUT_DSWISH) {
                    float a[4];
                    load4g(aux + row * C + ch, a);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] *= dswishf_(a[e]);
                    store4(y + row * C + ch, o);
                } else {
                    float a1[4], a2[4], o2[4];
                    load4g(aux + row * 2 * C + ch, a1);
                    load4g(aux + row * 2 * C + C + ch, a2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sg = sigmoidf_(a2[e]);
                        o2[e] = o[e] * a1[e] * sg * (1.f - sg);
                        o[e] *= sg;
                    }
                    store4(y + row * 2 * C + ch, o);
                    store4(y + row * 2 * C + C + ch, o2);
                }
            }
        }
    }
    if (ssum) {   // per-sample channel sums of this tile -> [B,C] (uniform branch)
        __syncthreads();
        float* red = tile;   // [8 tl][128 ch][2]
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[(tl * DW_CT + cl * 4 + e) * 2] = s1[e]; red[(tl * DW_CT + cl * 4 + e) * 2 + 1] = s2[e]; }
        __syncthreads();
        if (tid < DW_CT && c0 + tid < C) {
            float a = 0.f, q = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) { a += red[(r * DW_CT + tid) * 2]; q += red[(r * DW_CT + tid) * 2 + 1]; }
            if (part) {      // deterministic: this time tile's partial row [B][P = gridDim.x][2][C], summed by stats_reduce_kernel
                float* pr = part + (((size_t)b * gridDim.x + blockIdx.x) * 2) * C + c0 + tid;
                pr[0] = a; pr[C] = q;
            } else {
                atomicAdd(ssum + (size_t)b * C + c0 + tid, a);
                if (ssq) atomicAdd(ssq + (size_t)b * C + c0 + tid, q);
            }
        }
    }
}

// -------------------------------------------------------------------------------------
// Register-window variants for the kernel sizes the model uses (K in {3,5,11,15}): a thread
// owns 4 channels x DWR_SEG consecutive time steps of one sample, keeps the last K transformed
// inputs and the K taps in registers (slot indices are compile-time through a K-unrolled body),
// so every input element is loaded and activated once, there is no LDS tile and no barrier.
// -------------------------------------------------------------------------------------
#define DWR_SEG 32
#define DWR_SEG_SMALL 8      // dwconv_reg8_kernel at B <= DW_SMALL_B
#define DW_SMALL_B 8

// raw 4-channel load (value v, GLU gate g) and the input transform, kept separate so that a K-group's loads can all be
// issued before the first one is consumed
template <typename T>
DEVI void dw_raw(const T* __restrict__ x, int b, int tin, int Tn, int C, int Cin, int ch, int inop, float (&v)[4], float (&g)[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.f;
    g[0] = g[1] = g[2] = g[3] = 0.f;
    if (tin < 0 || tin >= Tn) return;
    const T* p = x + ((size_t)b * Tn + tin) * Cin + ch;
    load4g(p, v);
    if (inop == DWIN_GLU) load4g(p + C, g);
}
DEVI void dw_xform(int inop, float (&v)[4], const float (&g)[4]) {
    if (inop == DWIN_SWISH) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = swishf_(v[e]);
    } else if (inop == DWIN_GLU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] *= sigmoidf_(g[e]);
    }
}
template <typename T>
DEVI void dw_load_in(const T* __restrict__ x, int b, int tin, int Tn, int C, int Cin, int ch, int inop, float (&v)[4]) {
    float g[4];
    dw_raw(x, b, tin, Tn, C, Cin, ch, inop, v, g);
    dw_xform(inop, v, g);
}

template <typename T, int K>
__global__ __launch_bounds__(256) void dwconv_reg_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         T* __restrict__ y, const T* __restrict__ aux,
                                                         float* __restrict__ ssum, float* __restrict__ ssq,
                                                         int Tn, int C, int padl, int inop, int outop, int flip, float* __restrict__ part) {
    // workgroup = 64 channel quads (256 channels: one wave reads 512 contiguous bytes of a row) x 4 consecutive segments of
    // one sample: the per-(sample, channel) statistics of the 4 segments are combined in LDS before the atomics
    __shared__ float sred[4][64][8];
    const int cg = C >> 2;
    const int nseg = (Tn + DWR_SEG - 1) / DWR_SEG;
    const int ncb = (cg + 63) >> 6;
    const int c4 = (blockIdx.x % ncb) * 64 + (threadIdx.x & 63), seg = (blockIdx.x / ncb) * 4 + (threadIdx.x >> 6), b = blockIdx.y;
    const bool live = c4 < cg && seg < nseg;
    const int ch = min(c4, cg - 1) * 4;
    const int Cin = (inop == DWIN_GLU) ? 2 * C : C;
    float wr[K][4], win[K][4];
#pragma unroll
    for (int j = 0; j < K; ++j) load4(w + (size_t)(flip ? (K - 1 - j) : j) * C + ch, wr[j]);
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) load4(bias + ch, bv);
    const int t0 = seg * DWR_SEG, tend = live ? min(Tn, t0 + DWR_SEG) : t0;
    // slots 0..K-2 hold inputs t0-padl .. t0-padl+K-2
#pragma unroll
    for (int j = 0; j < K - 1; ++j) dw_load_in(x, b, t0 - padl + j, Tn, C, Cin, ch, inop, win[j]);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    constexpr int LB = K <= 5 ? K : 4;           // input rows whose loads are in flight together (K = 11, 15: batches of 4)
    for (int tb = t0; tb < tend; tb += K) {
#pragma unroll
      for (int u0 = 0; u0 < K; u0 += LB) {
        float nv[LB][4], ng[LB][4];
#pragma unroll
        for (int uu = 0; uu < LB; ++uu) dw_raw(x, b, (u0 + uu < K && tb + u0 + uu < tend) ? tb + u0 + uu - padl + K - 1 : -1, Tn, C, Cin, ch, inop, nv[uu], ng[uu]);
#pragma unroll
        for (int uu = 0; uu < LB; ++uu) {        // output t = tb + u uses slots (u + j) % K ; the new input lands in slot (u + K - 1) % K
            const int u = u0 + uu;
            const int t = tb + u;
            if (u < K && t < tend) {
                dw_xform(inop, nv[uu], ng[uu]);
#pragma unroll
                for (int e = 0; e < 4; ++e) win[(u + K - 1) % K][e] = nv[uu][e];
                float o[4] = {bv[0], bv[1], bv[2], bv[3]};
#pragma unroll
                for (int j = 0; j < K; ++j) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] += wr[j][e] * win[(u + j) % K][e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1[e] += o[e]; s2[e] += o[e] * o[e]; }
                const size_t row = (size_t)b * Tn + t;
                if (outop == OUT_NONE) {
                    store4(y + row * C + ch, o);
                } else if (outop == OUT_DSWISH) {
                    float a[4];
                    load4g(aux + row * C + ch, a);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] *= dswishf_(a[e]);
                    store4(y + row * C + ch, o);
                } else {
                    float a1[4], a2[4], o2[4];
                    load4g(aux + row * 2 * C + ch, a1);
                    load4g(aux + row * 2 * C + C + ch, a2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float sg = sigmoidf_(a2[e]);
                        o2[e] = o[e] * a1[e] * sg * (1.f - sg);
                        o[e] *= sg;
                    }
                    store4(y + row * 2 * C + ch, o);
                    store4(y + row * 2 * C + C + ch, o2);
                }
            }
        }
      }
    }
    if (ssum) {
        const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
#pragma unroll
        for (int e = 0; e < 4; ++e) { sred[sl][cl][e] = live ? s1[e] : 0.f; sred[sl][cl][4 + e] = live ? s2[e] : 0.f; }
        __syncthreads();
        if (sl == 0 && c4 < cg) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float a = 0.f, q = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) { a += sred[r][cl][e]; q += sred[r][cl][4 + e]; }
                if (part) {  // deterministic partial row of this 4-segment group: [B][P = gridDim.x / ncb][2][C]
                    const int P = gridDim.x / ncb, pi = blockIdx.x / ncb;
                    float* pr = part + (((size_t)b * P + pi) * 2) * C + ch + e;
                    pr[0] = a; pr[C] = q;
                } else {
                    atomicAdd(ssum + (size_t)b * C + ch + e, a);
                    if (ssq) atomicAdd(ssq + (size_t)b * C + ch + e, q);
                }
            }
        }
    }
}

// ---- forward only, 8 channels per lane (16-byte accesses: a wave reads / writes 1 KB of a row per instruction — the 8-byte kernel
// above tops out near 3.4 TB/s, tools/micro/load_pattern.hip / store_pattern.hip).  K = 3, 5; C % 8 == 0 with C / 8 a divisor of 256.
// Workgroup = C/8 lanes x (256 / (C/8)) consecutive 32-step segments of one sample; statistics as in dwconv_reg_kernel.
template <typename T>
DEVI void dw8_raw(const T* __restrict__ x, int b, int tin, int Tn, int C, int Cin, int ch, int inop, float (&v)[8], float (&g)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { v[e] = 0.f; g[e] = 0.f; }
    if (tin < 0 || tin >= Tn) return;
    const T* p = x + ((size_t)b * Tn + tin) * Cin + ch;
    load8(p, v);
    if (inop == DWIN_GLU) load8(p + C, g);
}
template <typename T, int K, int INOP>
__global__ __launch_bounds__(256) void dwconv_reg8_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                          T* __restrict__ y, int Tn, int C, int padl, float* __restrict__ part, int seglen) {
    constexpr int inop = INOP;
    extern __shared__ float sred8[];            // [segments per workgroup][C/8][16]
    const int cg = C >> 3, spw = 256 / cg;
    const int nseg = (Tn + seglen - 1) / seglen;      // seglen: DWR_SEG, or DWR_SEG_SMALL for a handful of samples (more, shorter chains)
    const int cl = threadIdx.x % cg, sl = threadIdx.x / cg;
    const int seg = blockIdx.x * spw + sl, b = blockIdx.y;
    const bool live = seg < nseg;
    const int ch = cl * 8;
    const int Cin = (inop == DWIN_GLU) ? 2 * C : C;
    float wr[K][8], win[K][8];
#pragma unroll
    for (int j = 0; j < K; ++j) { load4(w + (size_t)j * C + ch, *reinterpret_cast<float(*)[4]>(&wr[j][0])); load4(w + (size_t)j * C + ch + 4, *reinterpret_cast<float(*)[4]>(&wr[j][4])); }
    float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (bias) { load4(bias + ch, *reinterpret_cast<float(*)[4]>(&bv[0])); load4(bias + ch + 4, *reinterpret_cast<float(*)[4]>(&bv[4])); }
    const int t0 = seg * seglen, tend = live ? min(Tn, t0 + seglen) : t0;
    auto xform = [&](float (&v)[8], const float (&g)[8]) {
        if (inop == DWIN_SWISH) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = swishf_(v[e]);
        } else if (inop == DWIN_GLU) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] *= sigmoidf_(g[e]);
        }
    };
#pragma unroll
    for (int j = 0; j < K - 1; ++j) { float g8[8]; dw8_raw(x, b, live ? t0 - padl + j : -1, Tn, C, Cin, ch, inop, win[j], g8); xform(win[j], g8); }
    float s1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, s2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    // Two groups of K input rows in flight (ping-pong register sets of RAW 16-byte rows): with one group the kernel is bound by
    // memory latency x bytes in flight (12 waves per CU x 64 lanes x K x 16 B: 3.7 TB/s by Little's law, as measured)
    typedef __attribute__((ext_vector_type(4))) uint32_t raw4;
    struct Grp { raw4 v[K], g[INOP == DWIN_GLU ? K : 1]; };
    Grp ga, gb;
    auto issue = [&](Grp& G, int tb) {
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const int tin = tb + u - padl + K - 1;
            G.v[u] = raw4{0u, 0u, 0u, 0u};
            if (INOP == DWIN_GLU) G.g[u] = raw4{0u, 0u, 0u, 0u};
            if (tb + u < tend && tin >= 0 && tin < Tn) {
                const T* p = x + ((size_t)b * Tn + tin) * Cin + ch;
                G.v[u] = *reinterpret_cast<const raw4*>(p);
                if (INOP == DWIN_GLU) G.g[u] = *reinterpret_cast<const raw4*>(p + C);
            }
        }
    };
    auto unpack = [&](const raw4& r, float (&v)[8]) {
        T tmp[8];
        *reinterpret_cast<raw4*>(tmp) = r;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = to_f(tmp[e]);
    };
    auto process = [&](const Grp& G, int tb) {
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const int t = tb + u;
            if (t < tend) {
                float nv[8], ng[8];
                unpack(G.v[u], nv);
                if (INOP == DWIN_GLU) unpack(G.g[INOP == DWIN_GLU ? u : 0], ng);
                xform(nv, ng);
#pragma unroll
                for (int e = 0; e < 8; ++e) win[(u + K - 1) % K][e] = nv[e];
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = bv[e];
#pragma unroll
                for (int j = 0; j < K; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] += wr[j][e] * win[(u + j) % K][e];
#pragma unroll
                for (int e = 0; e < 8; ++e) { s1[e] += o[e]; s2[e] += o[e] * o[e]; }
                store8(y + ((size_t)b * Tn + t) * C + ch, o);
            }
        }
    };
    issue(ga, t0);
    for (int tb = t0; tb < tend; tb += 2 * K) {
        issue(gb, tb + K);
        process(ga, tb);
        issue(ga, tb + 2 * K);
        process(gb, tb + K);
    }
    if (part) {     // deterministic partial row of this workgroup's segments: part[B][P = gridDim.x][2][C]
        float* sr = sred8 + ((size_t)sl * cg + cl) * 16;
#pragma unroll
        for (int e = 0; e < 8; ++e) { sr[e] = live ? s1[e] : 0.f; sr[8 + e] = live ? s2[e] : 0.f; }
        __syncthreads();
        if (sl == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float a = 0.f, q = 0.f;
                for (int r = 0; r < spw; ++r) { a += sred8[((size_t)r * cg + cl) * 16 + e]; q += sred8[((size_t)r * cg + cl) * 16 + 8 + e]; }
                float* pr = part + (((size_t)b * gridDim.x + blockIdx.x) * 2) * C + ch + e;
                pr[0] = a; pr[C] = q;
            }
        }
    }
}

// ---- forward, K = 11 / 15 (the first Conv1DBlock of a group, the transformer blocks' conv modules): a STREAMING LDS kernel.
// The 64 x 128 tile kernel above re-stages a (64 + K - 1)-row tile per workgroup (23 % halo at K = 15), runs load -> barrier -> compute -> store
// strictly in sequence inside a workgroup, and stores 8 bytes per lane: 2.6 TB/s at K = 11.  Here a workgroup owns 128 channels of ONE sample for
// a whole time range and walks it in 32-row chunks through a 64-row LDS ring of TRANSFORMED inputs (fp32, Swish / GLU applied once per element):
//   * no halo re-reads inside a range, the tap weights (K x 4 channels per thread) are loaded once per workgroup;
//   * the next chunk's global loads are in flight while the current chunk is computed (two barriers per chunk);
//   * (channel pairs as float2 / v_pk_fma_f32 were tried: forward depthwise conv 0.897 -> 1.087 ms/step — scalar FMAs stay)
//   * thread = 4 channels x 4 consecutive rows, row-stationary accumulation (every ring row is read once per thread and feeds up to four outputs);
//   * lane pairs swap halves (DPP quad_perm) so that every store is 16 bytes: an even lane writes 8 channels of rows 0 / 2, an odd lane of rows 1 / 3;
//   * BatchNorm / GAP statistics: per-thread sums over the whole range, one partial row per workgroup at the end (deterministic, as before).
// Non-causal convolutions (padl < K - 1) compute output row t when input row t + K - 1 - padl is in the ring: the output window lags the input
// window by `lag` rows and one more (input-free) chunk drains it.
template <typename T, int K, int INOP>
__global__ __launch_bounds__(256, 3) void dwconv_stream_kernel(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                                             T* __restrict__ y, int Tn, int C, int padl, float* __restrict__ part, int tsplit) {
    constexpr int RB = 64, CH = 32, CT = 128;           // ring rows, chunk rows, channels per workgroup
    __shared__ __attribute__((aligned(16))) float ring[RB * CT];
    __shared__ float sred[8][2][CT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c0 = blockIdx.x * CT, b = blockIdx.y;
    const int Cin = (INOP == DWIN_GLU) ? 2 * C : C;
    const int lag = K - 1 - padl;
    // time range of this workgroup (tsplit ranges per sample, multiples of CH rows)
    const int per = ((Tn + tsplit - 1) / tsplit + CH - 1) / CH * CH;
    const int r_beg = blockIdx.z * per, r_end = min(Tn, r_beg + per);
    if (r_beg >= Tn) return;
    // ---- compute mapping: 32 channel quads x 8 row groups of 4
    const int cq = tid & 31, rg = tid >> 5;
    const int ch = c0 + cq * 4;
    float wr[K][4];
#pragma unroll
    for (int j = 0; j < K; ++j) load4(w + (size_t)j * C + ch, wr[j]);
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias) load4(bias + ch, bv);
    float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
    // ---- staging mapping: 16 chunks of 8 channels x 16 rows, two row sets per chunk of 32 rows
    const int sc = tid & 15, sr = tid >> 4;
    typedef __attribute__((ext_vector_type(4))) uint32_t raw4;
    raw4 rv[2], rgl[2];
    auto gload = [&](int t0, bool hi_only = false) {           // input rows t0 .. t0+31 (zero outside [0, Tn); hi_only: rows t0+16 .. only — the K - 1 <= 14 history rows)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = t0 + sr + 16 * h;
            rv[h] = raw4{0u, 0u, 0u, 0u}; rgl[h] = raw4{0u, 0u, 0u, 0u};
            if (t >= 0 && t < Tn && (h == 1 || !hi_only)) {
                const T* p = x + ((size_t)b * Tn + t) * Cin + c0 + sc * 8;
                rv[h] = *reinterpret_cast<const raw4*>(p);
                if (INOP == DWIN_GLU) rgl[h] = *reinterpret_cast<const raw4*>(p + C);
            }
        }
    };
    auto lstore = [&](int t0) {          // transform once, fp32 into the ring slot of the row
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = t0 + sr + 16 * h;
            float v[8];
            { T tmp[8]; *reinterpret_cast<raw4*>(tmp) = rv[h];
#pragma unroll
              for (int e = 0; e < 8; ++e) v[e] = to_f(tmp[e]); }
            if (INOP == DWIN_SWISH) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = swishf_(v[e]);
            } else if (INOP == DWIN_GLU) {
                T tg[8]; *reinterpret_cast<raw4*>(tg) = rgl[h];
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= sigmoidf_(to_f(tg[e]));
            }
            if (t < 0 || t >= Tn) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = 0.f;
            }
            float* dst = ring + ((t & (RB - 1)) * CT) + sc * 8;
            *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
    };
    // prologue: the history rows [in0 - CH, in0) (zeros before the sample / real rows when a range starts inside it) and the first chunk
    const int in0 = (r_beg + lag) / CH * CH;            // output row t is computed by the chunk that brings input row t + lag
    gload(in0 - CH, true); lstore(in0 - CH);
    gload(in0); lstore(in0);
    __syncthreads();
    // chunk i: inputs [ti, ti + CH) are in the ring; outputs [ti - lag, ti + CH - lag) clipped to [r_beg, r_end)
    for (int ti = in0; ti - lag < r_end; ti += CH) {
        const bool more = ti + CH - lag < r_end;
        if (more) gload(ti + CH);
        const int o0 = ti - lag + rg * 4;                 // first output row of this thread
        float acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[u][e] = 0.f;
        // input rows o0 - padl .. o0 - padl + K + 2
#pragma unroll
        for (int qd = 0; qd < K + 3; ++qd) {
            const int tin = o0 - padl + qd;
            const float4 rw = *reinterpret_cast<const float4*>(ring + ((tin & (RB - 1)) * CT) + cq * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = qd - u;
                if (j >= 0 && j < K) { acc[u][0] += wr[j][0] * rw.x; acc[u][1] += wr[j][1] * rw.y; acc[u][2] += wr[j][2] * rw.z; acc[u][3] += wr[j][3] * rw.w; }
            }
        }
        // pack, swap halves inside lane pairs, 16-byte stores
        uint32_t pk[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool live = o0 + u >= r_beg && o0 + u < r_end;
#pragma unroll
            for (int e = 0; e < 4; ++e) { acc[u][e] += bv[e]; if (live) { s1[e] += acc[u][e]; s2[e] += acc[u][e] * acc[u][e]; } }
            T tmp[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) tmp[e] = from_f<T>(acc[u][e]);
            pk[u][0] = reinterpret_cast<const uint32_t*>(tmp)[0]; pk[u][1] = reinterpret_cast<const uint32_t*>(tmp)[1];
        }
        const bool odd = lane & 1;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // even lane keeps rows 2h (own low half | partner's half), odd lane rows 2h + 1 (partner's half | own high half)
            const int mine = 2 * h + (odd ? 1 : 0), theirs = 2 * h + (odd ? 0 : 1);
            uint32_t give0 = pk[theirs][0], give1 = pk[theirs][1];
            const uint32_t got0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)give0, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
            const uint32_t got1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)give1, 0xB1, 0xf, 0xf, true);
            const int t = o0 + mine;
            if (t >= r_beg && t < r_end) {
                raw4 o = odd ? raw4{got0, got1, pk[mine][0], pk[mine][1]} : raw4{pk[mine][0], pk[mine][1], got0, got1};
                *reinterpret_cast<raw4*>(y + ((size_t)b * Tn + t) * C + c0 + (cq >> 1) * 8) = o;
            }
        }
        __syncthreads();                 // every thread is done reading the rows the next chunk overwrites
        if (more) lstore(ti + CH);
        __syncthreads();
    }
    if (part) {      // one partial row per (sample, time range): part[B][P = tsplit][2][C]
        sred[rg][0][cq * 4 + 0] = s1[0]; sred[rg][0][cq * 4 + 1] = s1[1]; sred[rg][0][cq * 4 + 2] = s1[2]; sred[rg][0][cq * 4 + 3] = s1[3];
        sred[rg][1][cq * 4 + 0] = s2[0]; sred[rg][1][cq * 4 + 1] = s2[1]; sred[rg][1][cq * 4 + 2] = s2[2]; sred[rg][1][cq * 4 + 3] = s2[3];
        __syncthreads();
        if (tid < CT) {
            float a = 0.f, q = 0.f;
#pragma unroll
            for (int r = 0; r < 8; ++r) { a += sred[r][0][tid]; q += sred[r][1][tid]; }
            float* pr = part + (((size_t)b * gridDim.z + blockIdx.z) * 2) * C + c0 + tid;
            pr[0] = a; pr[C] = q;
        }
    }
}

// ---- Which kernel runs.  dwconv_fwd_route / dwconv_bwd_route decide, here and nowhere else: they alone read the switches (g_force_dw_lds,
// ISHARA_NO_DW_STREAM) and hold the applicability tests; the launchers launch what they return and dwconv_*_kernel_name names it.
// A new kernel gets an enumerator, its test in the route (in priority order) and a case in the launcher's switch and the name's switch.
int g_force_dw_lds = 0;    // tests: force the LDS-tiled kernels

static bool dw_shape_ok(int C, int k) { return C % 8 == 0 && k >= 1 && k <= DW_MAXK; }
static int dwconv_check(int C, int k) {
    if (dw_shape_ok(C, k)) return 0;
    if (C % 8 != 0) ishara_set_error("dwconv: C=%d must be a multiple of 8", C);
    else ishara_set_error("dwconv: kernel size %d unsupported (1..%d)", k, DW_MAXK);
    return -1;
}
// the kernel sizes the model uses have kernels instantiated for them (a K-unrolled body): 3 / 5 a register window, 11 / 15 the streaming
// forward, all four the one-pass backward and the windowed weight gradient
static bool dw_k_small(int k) { return k == 3 || k == 5; }
static bool dw_k_wide(int k) { return k == 11 || k == 15; }
static bool dw_k_unrolled(int k) { return dw_k_small(k) || dw_k_wide(k); }
// dwconv_reg_kernel (forward and data gradient): C/4 lanes a divisor of 256.  K = 11, 15: the register window (201 / 233 VGPRs) measured
// 94 / 103 us vs 82 / 86 us for the LDS-tiled kernel
static bool dw_reg_ok(int C, int k) { return dw_k_small(k) && C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0; }
// dwconv_reg8_kernel's segment: a handful of samples (B = 1 inference) takes 8-step segments — four times the workgroups, a quarter of the
// dependent steps per thread (3 workgroups of 32-step chains took 17 us at T = 384)
static int dw_reg8_seglen(int B) { return B <= DW_SMALL_B ? DWR_SEG_SMALL : DWR_SEG; }

DwFwdRoute dwconv_fwd_route(int dt, int B, int T, int C, int k, bool stats, bool part) {
    if (!dw_shape_ok(C, k)) return DWF_REFUSED;
    if (g_force_dw_lds) return DWF_TILE;
    static const bool no_stream = getenv("ISHARA_NO_DW_STREAM") != nullptr;      // A/B switch: the 64 x 128 tile kernel instead
    const bool b16 = dt != DT_F32;
    const bool rows = part || !stats;          // the streaming and 8-channel kernels give statistics only through the deterministic partial rows
    // 16-bit storage, whole 128-channel workgroups, at least two 32-row chunks; a handful of samples has too few workgroups for it
    if (b16 && dw_k_wide(k) && C % 128 == 0 && T >= 64 && B > DW_SMALL_B && !no_stream && rows) return DWF_STREAM;
    // 16-bit storage, C/8 in {32, 64, 128, 256}
    if (b16 && dw_k_small(k) && C / 8 >= 32 && C / 8 <= 256 && 256 % (C / 8) == 0 && rows) return DWF_REG8;
    if (dw_reg_ok(C, k)) return DWF_REG;
    return DWF_TILE;
}

DwBwdRoute dwconv_bwd_route(int dt, int C, int k, int padl, bool scratch, bool bn) {
    DwBwdRoute r = {DWB_TWO_PASS, DWD_TILE, DWW_TILE_ATOMIC};
    if (!dw_shape_ok(C, k)) { r.kind = DWB_REFUSED; return r; }
    if (g_force_dw_lds) return r;
    // one pass (dwconv_bwd.hip): partial rows need the scratch; fp32 rows would need K * 4 more registers for the window
    if (scratch && dw_k_unrolled(k) && (dt == DT_BF16 || k <= 5) && C % 4 == 0 && C / 4 <= 256 && padl >= 0 && padl < k) {
        r.kind = bn && k < 15 ? DWB_FUSED_BN : DWB_FUSED;      // k = 15: the 15-row window + the BatchNorm coefficients spill (26+ VGPRs)
        return r;
    }
    if (dw_reg_ok(C, k)) r.dgrad = DWD_REG;
    if (scratch) r.wgrad = dw_k_unrolled(k) ? DWW_WIN : DWW_TILE_PART;      // partial rows when the caller gave room for them (DWG_BLOCKS rows), else atomics
    return r;
}

// The partial statistic rows per sample the forward kernel of `route` writes for (B, T, C), which is also the time extent of its grid: every
// forward launcher builds its grid on this, and a caller that sums the rows itself (part_rows of launch_dwconv_fwd) knows the count before
// the launch.  tsplit: the streaming kernel's time ranges per sample.
int dwconv_fwd_part_rows(DwFwdRoute route, int B, int T, int C, int* tsplit) {
    switch (route) {
        case DWF_REFUSED: break;
        case DWF_STREAM: {
            // enough workgroups for ~3 rounds of the chip's 768-1024 slots, whole 32-row chunks per range
            int ts = 1;
            while ((C / 128) * B * ts < 2048 && T / (ts * 2) >= 128) ts *= 2;      // every extra range re-reads 16 history rows
            if (tsplit) *tsplit = ts;
            // The kernel rounds a range up to whole chunks (`per`, computed here as there), so the last of the tsplit ranges can begin past the end
            // (T = 1025..1120: 8 ranges of 160 rows).  Such a range is not launched and not counted: its workgroup would return without writing its
            // partial row.  The kernel still gets tsplit, so every launched workgroup has the range it always had.
            const int per = ((T + ts - 1) / ts + 31) / 32 * 32;
            return (T + per - 1) / per;
        }
        case DWF_REG8: {
            const int seglen = dw_reg8_seglen(B), spw = 256 / (C / 8), nseg = (T + seglen - 1) / seglen;
            return (nseg + spw - 1) / spw;
        }
        case DWF_REG: return ((T + DWR_SEG - 1) / DWR_SEG + 3) / 4;
        case DWF_TILE: return (T + DW_TT - 1) / DW_TT;
    }
    return 0;
}

static const char* dw_tile_name(int k) { return k == 11 ? "dwconv_kernel<11,11>" : (k <= 15 ? "dwconv_kernel<0,15>" : "dwconv_kernel<0,31>"); }
// the prefix of the rocprof name of the kernel launch_dwconv_fwd launches for the same arguments (the tile kernel with its <KC,KM> variant); "" when refused
const char* dwconv_fwd_kernel_name(int dt, int B, int T, int C, int k, bool stats, bool part) {
    switch (dwconv_fwd_route(dt, B, T, C, k, stats, part)) {
        case DWF_REFUSED: return "";
        case DWF_STREAM: return "dwconv_stream_kernel";
        case DWF_REG8: return "dwconv_reg8_kernel";
        case DWF_REG: return "dwconv_reg_kernel";
        case DWF_TILE: return dw_tile_name(k);
    }
    return "";
}
// the same for launch_dwconv_bwd_bn (bn) / launch_dwconv_bwd; the one-pass kernel as <BN> when it folds the BatchNorm backward, a two-pass backward as dgrad+wgrad
const char* dwconv_bwd_kernel_name(int dt, int C, int k, int padl, bool scratch, bool bn) {
    static char name[96];
    const DwBwdRoute r = dwconv_bwd_route(dt, C, k, padl, scratch, bn);
    switch (r.kind) {
        case DWB_REFUSED: return "";
        case DWB_FUSED_BN: return "dwconv_bwd_fused_kernel<BN>";
        case DWB_FUSED: return "dwconv_bwd_fused_kernel";
        case DWB_TWO_PASS: break;
    }
    static const char* const wg[] = {"dwconv_wgrad_win_kernel", "dwconv_wgrad_kernel<part>", "dwconv_wgrad_kernel<atomic>"};      // by DwWgrad
    snprintf(name, sizeof name, "%s+%s", r.dgrad == DWD_REG ? "dwconv_reg_kernel" : dw_tile_name(k), wg[r.wgrad]);
    return name;
}

// ---- kernel launches.  The forward ones return the partial statistic rows per sample they write.
// fn(T{}) in the storage type dt: the 16-bit types / all three / the two of the backward pass
template <typename F> static int dw_typed16(int dt, F fn) { return dt == DT_BF16 ? fn(bf16{}) : fn(f16{}); }
template <typename F> static int dw_typed(int dt, F fn) { return dt == DT_F32 ? fn(float{}) : dw_typed16(dt, fn); }
template <typename F> static int dw_typed_bwd(int dt, F fn) { return dt == DT_BF16 ? fn(bf16{}) : fn(float{}); }
template <typename T>
static int launch_dw_stream(int k, const T* x, const float* w, const float* bias, T* y, int B, int Tn, int C, int padl, int inop, float* part, hipStream_t s) {
    int tsplit = 1;
    const int ranges = dwconv_fwd_part_rows(DWF_STREAM, B, Tn, C, &tsplit);
    const dim3 grid(C / 128, B, ranges);
#define DWS(KK, OP) hipLaunchKernelGGL((dwconv_stream_kernel<T, KK, OP>), grid, dim3(256), 0, s, x, w, bias, y, Tn, C, padl, part, tsplit)
#define DWSK(OP) do { if (k == 11) DWS(11, OP); else DWS(15, OP); } while (0)
    if (inop == DWIN_SWISH) DWSK(DWIN_SWISH); else if (inop == DWIN_GLU) DWSK(DWIN_GLU); else DWSK(DWIN_NONE);
#undef DWSK
#undef DWS
    return ranges;
}

template <typename T>
static int launch_dw_reg8(int k, const T* x, const float* w, const float* bias, T* y, int B, int Tn, int C, int padl, int inop, float* part, hipStream_t s) {
    const int seglen = dw_reg8_seglen(B);
    const dim3 grid(dwconv_fwd_part_rows(DWF_REG8, B, Tn, C), B);
    const size_t sh = (size_t)256 * 16 * sizeof(float);
#define DW8(KK, OP) hipLaunchKernelGGL((dwconv_reg8_kernel<T, KK, OP>), grid, dim3(256), sh, s, x, w, bias, y, Tn, C, padl, part, seglen)
#define DW8K(OP) do { if (k == 3) DW8(3, OP); else DW8(5, OP); } while (0)
    if (inop == DWIN_SWISH) DW8K(DWIN_SWISH); else if (inop == DWIN_GLU) DW8K(DWIN_GLU); else DW8K(DWIN_NONE);
#undef DW8K
#undef DW8
    return (int)grid.x;
}

template <typename T>
static int launch_dw_reg(int k, const T* x, const float* w, const float* bias, T* y, const T* aux, float* ssum, float* ssq,
                         int B, int Tn, int C, int padl, int inop, int outop, int flip, hipStream_t s, float* part = nullptr) {
    const int rows = dwconv_fwd_part_rows(DWF_REG, B, Tn, C);
    dim3 grid(((C / 4 + 63) / 64) * rows, B);
#define DWR(KK) hipLaunchKernelGGL((dwconv_reg_kernel<T, KK>), grid, dim3(256), 0, s, x, w, bias, y, aux, ssum, ssq, Tn, C, padl, inop, outop, flip, part)
    switch (k) { case 3: DWR(3); break; case 5: DWR(5); break; case 11: DWR(11); break; default: DWR(15); break; }
#undef DWR
    return rows;
}

template <typename T>
static int launch_dw_tile(const T* x, const float* w, const float* bias, T* y, const T* aux, float* ssum, float* ssq,
                          int B, int Tn, int C, int k, int padl, int inop, int outop, int flip, hipStream_t s, float* part = nullptr) {
    dim3 grid(dwconv_fwd_part_rows(DWF_TILE, B, Tn, C), (C + DW_CT - 1) / DW_CT, B);
#define DWK(KC, KM) hipLaunchKernelGGL((dwconv_kernel<T, KC, KM>), grid, dim3(256), 0, s, x, w, bias, y, aux, ssum, ssq, B, Tn, C, k, padl, inop, outop, flip, part)
    if (k == 11) DWK(11, 11);            // 74 -> 65 us
    else if (k <= 15) DWK(0, 15);        // K = 15 unrolled: 86 vs 78 us
    else DWK(0, DW_MAXK);
#undef DWK
    return (int)grid.x;
}

// ssum / ssq [B, C] = per-sample channel sums of the partial rows part[B][P][2][C], in a fixed order (no float atomics:
// the forward pass is bit-reproducible run to run, and no zero-fill launches are needed)
__global__ __launch_bounds__(256) void stats_reduce_kernel(const float* __restrict__ part, int P, float* __restrict__ ssum, float* __restrict__ ssq, int B, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * C) return;
    const int b = i / C, c = i - b * C;
    const float* p = part + ((size_t)b * P * 2) * C + c;
    float a = 0.f, q = 0.f;
    for (int r = 0; r < P; ++r) { a += p[(size_t)(2 * r) * C]; q += p[(size_t)(2 * r + 1) * C]; }
    ssum[i] = a;
    if (ssq) ssq[i] = q;
}
size_t dwconv_fwd_scratch_floats(int B, int T, int C) {
    const size_t big = (size_t)B * ((T + DWR_SEG - 1) / DWR_SEG), small = (size_t)(B < DW_SMALL_B ? B : DW_SMALL_B) * ((T + DWR_SEG_SMALL - 1) / DWR_SEG_SMALL);
    return (big > small ? big : small) * 2 * C;
}   // the most partial rows any forward kernel writes per sample (one per 32-step segment)
size_t dwconv_bwd_scratch_floats(int C, int k) { return (size_t)DWG_BLOCKS * (k + 1) * C; }

// `part`: scratch of dwconv_fwd_scratch_floats(B, T, C) floats for the deterministic statistics, or nullptr (then colsum /
// colsq must be zero-filled by the caller and are accumulated with float atomics)
int launch_dwconv_fwd(int dt, int inop, const void* x, const float* w, const float* bias, void* y,
                      float* colsum, float* colsq, float* part, int B, int T, int C, int k, int padl, hipStream_t s, int* part_rows) {
    if (dwconv_check(C, k)) return -1;
    if (!colsum) part = nullptr;
    int P = 0;
    switch (dwconv_fwd_route(dt, B, T, C, k, colsum != nullptr, part != nullptr)) {
        case DWF_REFUSED: return -1;      // dwconv_check has said why
        case DWF_STREAM: P = dw_typed16(dt, [&](auto t) { using TT = decltype(t); return launch_dw_stream<TT>(k, (const TT*)x, w, bias, (TT*)y, B, T, C, padl, inop, part, s); }); break;
        case DWF_REG8: P = dw_typed16(dt, [&](auto t) { using TT = decltype(t); return launch_dw_reg8<TT>(k, (const TT*)x, w, bias, (TT*)y, B, T, C, padl, inop, part, s); }); break;
        case DWF_REG: P = dw_typed(dt, [&](auto t) { using TT = decltype(t); return launch_dw_reg<TT>(k, (const TT*)x, w, bias, (TT*)y, nullptr, colsum, colsq, B, T, C, padl, inop, OUT_NONE, 0, s, part); }); break;
        case DWF_TILE: P = dw_typed(dt, [&](auto t) { using TT = decltype(t); return launch_dw_tile<TT>((const TT*)x, w, bias, (TT*)y, nullptr, colsum, colsq, B, T, C, k, padl, inop, OUT_NONE, 0, s, part); }); break;
    }
    if (part && part_rows) *part_rows = P;          // the caller sums the partial rows itself (eca_fwd's inference form)
    else if (part) hipLaunchKernelGGL(stats_reduce_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, P, colsum, colsq, B, C);
    return launch_rc();
}

// dw [k, C] and dbias [C] += the column sums of `rows` partial rows [(k + 1) * C] (dw then dbias)
static void dw_sum_rows(const float* part, int rows, float* dw, float* dbias, int C, int k, hipStream_t s) {
    launch_reduce_slabs(part, dw, k * C, rows, (size_t)(k + 1) * C, s);
    if (dbias) launch_reduce_slabs(part + (size_t)k * C, dbias, C, rows, (size_t)(k + 1) * C, s);
}

int launch_dwconv_bwd_bn(int dt, int inop, const void* dy, const DwBnArgs& bn, const void* x, const float* w, void* dx,
                         float* dw, float* dbias, float* scratch, int B, int T, int C, int k, int padl, hipStream_t s) {
    if (dwconv_check(C, k)) return -1;
    if (dwconv_bwd_route(dt, C, k, padl, scratch != nullptr, bn.h != nullptr).kind != DWB_FUSED_BN) return 0;
    const int rows = launch_dwconv_bwd_fused(dt, inop, dy, x, w, dx, scratch, B, T, C, k, padl, DWG_BLOCKS, s, bn);
    if (rows < 0) return -2;
    dw_sum_rows(scratch, rows, dw, dbias, C, k, s);
    return hipGetLastError() == hipSuccess ? 1 : -2;
}

int launch_dwconv_bwd(int dt, int inop, const void* dy, const void* x, const float* w, void* dx,
                      float* dw, float* dbias, float* scratch, int B, int T, int C, int k, int padl, hipStream_t s) {
    if (dwconv_check(C, k)) return -1;
    const DwBwdRoute r = dwconv_bwd_route(dt, C, k, padl, scratch != nullptr, false);
    int rows = 0;
    switch (r.kind) {
        case DWB_REFUSED: case DWB_FUSED_BN: return -1;      // dwconv_check has said why; no BatchNorm was asked for
        case DWB_FUSED:      // one pass: dx and the per-workgroup partial rows of (dw, dbias), then the row sum
            rows = launch_dwconv_bwd_fused(dt, inop, dy, x, w, dx, scratch, B, T, C, k, padl, DWG_BLOCKS, s, DwBnArgs());
            if (rows < 0) return -2;
            dw_sum_rows(scratch, rows, dw, dbias, C, k, s);
            return launch_rc();
        case DWB_TWO_PASS: break;
    }
    // data grad: correlation with flipped taps, left pad k-1-padl; then through the input op
    const int outop = inop == DWIN_SWISH ? OUT_DSWISH : (inop == DWIN_GLU ? OUT_DGLU : OUT_NONE);
    switch (r.dgrad) {
        case DWD_REG: dw_typed_bwd(dt, [&](auto t) { using TT = decltype(t); return launch_dw_reg<TT>(k, (const TT*)dy, w, nullptr, (TT*)dx, (const TT*)x, nullptr, nullptr, B, T, C, k - 1 - padl, DWIN_NONE, outop, 1, s); }); break;
        case DWD_TILE: dw_typed_bwd(dt, [&](auto t) { using TT = decltype(t); return launch_dw_tile<TT>((const TT*)dy, w, nullptr, (TT*)dx, (const TT*)x, nullptr, nullptr, B, T, C, k, k - 1 - padl, DWIN_NONE, outop, 1, s); }); break;
    }
    // weight / bias grad: through per-workgroup partial rows in the scratch, or with atomics
    rows = launch_dwconv_wgrad(r.wgrad, dt, inop, dy, x, dw, dbias, r.wgrad == DWW_TILE_ATOMIC ? nullptr : scratch, B, T, C, k, padl, s);
    if (rows) dw_sum_rows(scratch, rows, dw, dbias, C, k, s);
    return launch_rc();
}
