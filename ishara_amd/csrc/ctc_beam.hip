// CTC prefix beam search with an optional character-bigram LM (shallow fusion): the semantics of ishara_amd/ctc_beam.py, on the device.
//
// One workgroup per clip, looping over the T frames; NW = min(16, pow2ceil(W)) wavefronts.  Per frame:
//   1. merge detection (all threads, one (i, j) beam pair per step): the extension of beam i by last(j) is beam j's prefix when
//      len_j = len_i + 1, hash(prefix_j[:-1]) = hash(prefix_i) (64-bit polynomial hash, a filter only) and prefix_j's parent node is node_i
//      (kept in LDS), or else the trie chains agree character by character (exact; a prefix that was pruned and re-created has a new trie
//      node while a surviving child still points at the old one, so node ids alone are not identity; only then is global memory read).
//   2. candidates (wave w owns beams w, w + NW, ...; lane c = class c): lane b carries the same-prefix candidate (with the merged extension
//      term), lane c != b the extension by c (none if merged).  Each candidate is one 64-bit key: the score mapped to an order-preserving
//      uint32 in the high word, the complement of (kind, source beam, class) in the low word, so a larger key is exactly "earlier in the
//      total order".  The wave sorts its 64 keys (bitonic, xor shuffles) and merges the top 32 into its running list (bitonic merge).
//   3. the NW lists are merged pairwise through LDS in log2(NW) rounds; wave 0 ends with the global top W in rank order.
//   4. wave 0 writes the new beams (double-buffered state in LDS), appends extension nodes to the clip's trie in the workspace and
//      renormalises: the acoustic and LM/length parts are kept relative to the top beam, with the offsets summed in fp64, so the fp32
//      beam values stay small; the device scores agree with the fp64 host reference within 1e-3 at T = 384 (tests/test_ctc_beam_gpu.py).
// The log-softmax of up to BM_CHUNK frames at a time is staged in LDS from logits loaded one chunk ahead; the LM table is staged once.
// No atomics: runs are bit-reproducible.
//
// AUT (ishara_ctc_beam_decode_lm): the LM is a deterministic automaton, logp [S, C] f32 and next [S, C] i32 in global memory, and every beam
// carries its state.  The 16 KB of LDS that hold the [C, C] table hold instead, per beam, the logp row and the next row of its state (32 x 64
// f32 + 32 x 64 i32).  Wave w owns the rows of beams w, w + NW, ... (the beams whose candidates it forms in 2.): at the top of a frame it
// issues the two coalesced row loads of each of its beams into registers, the chunk's log-softmax and merge detection (1.) run under them,
// and the rows are written to LDS just before the barrier that ends 1.  A beam that stayed at its rank with its prefix keeps its rows (no
// load).  The extension term is formed by bm_ext_bonus exactly as for the table, so a bigram automaton gives the table kernel's bits; the
// table instantiations compile none of this (every statement of it is under `if constexpr (AUT)`).
#include "kernels.h"

#define BM_MAXC 64
#define BM_MAXW 32
#define BM_MAXNW 16
#define BM_CHUNK 16
#define BM_PRE 4                   // frames of logits per wave loaded ahead (the chunk is min(BM_CHUNK, BM_PRE * NW) frames)
#define BM_NEG (-__builtin_inff())
#define BM_HASH_MUL 0x9E3779B97F4A7C15ull
#define BM_LMPER (BM_MAXW / BM_MAXNW)                       // AUT: beams per wave at most (the launch has NW >= W or NW = BM_MAXNW)
#define BM_LMHELD ((int)0x80000000)                         // AUT: bit 31 of BmState.lmstate

typedef unsigned long long u64;

// trie node word in the workspace: parent node (bits 0..23) | class (bits 24..29); node 0 is the empty prefix
__host__ __device__ size_t ctc_beam_workspace_words(int T, int W) { return 1 + (size_t)T * W; }

// log(e^a + e^b); -inf (+) -inf = -inf.  Explicitly rounded operations everywhere a score is formed, so the candidate pass and the
// state update (different inlining contexts) produce the same bits.
DEVI float bm_lse(float a, float b) {
    const float m = fmaxf(a, b);
    if (m == BM_NEG) return BM_NEG;
    return __fadd_rn(m, log1pf(expf(-fabsf(__fsub_rn(a, b)))));
}
DEVI uint32_t bm_ord(float s) {                            // order-preserving float -> uint32 (-0 folded onto +0 first)
    uint32_t u = __float_as_uint(__fadd_rn(s, 0.0f));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DEVI u64 bm_key(float s, int kind, int src, int c) {
    return ((u64)bm_ord(s) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)((kind << 16) | (src << 8) | c));
}
DEVI u64 bm_shfl(u64 v, int src) {
    const int lo = __shfl((int)(uint32_t)v, src), hi = __shfl((int)(uint32_t)(v >> 32), src);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}
DEVI u64 bm_shfl_xor(u64 v, int m) {
    const int lo = __shfl_xor((int)(uint32_t)v, m), hi = __shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}
DEVI u64 bm_max(u64 a, u64 b) { return a > b ? a : b; }
DEVI u64 bm_min(u64 a, u64 b) { return a < b ? a : b; }
// descending bitonic sort of one key per lane over the wave
DEVI u64 bm_sort64(u64 v, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const u64 o = bm_shfl_xor(v, j);
            const bool keep_max = ((lane & j) == 0) == ((lane & k) == 0);
            v = keep_max ? bm_max(v, o) : bm_min(v, o);
        }
    }
    return v;
}
// lanes 0..31 descending, lanes 32..63 ascending (a bitonic sequence) -> descending over the wave
DEVI u64 bm_merge64(u64 v, int lane) {
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) {
        const u64 o = bm_shfl_xor(v, j);
        v = (lane & j) == 0 ? bm_max(v, o) : bm_min(v, o);
    }
    return v;
}
DEVI float bm_ext_bonus(float bonus, float lmv, float alpha, float beta, bool use_lm) {
    return __fadd_rn(use_lm ? __fadd_rn(bonus, __fmul_rn(alpha, lmv)) : bonus, beta);
}

struct BmState {
    float pb[BM_MAXW], pnb[BM_MAXW], bonus[BM_MAXW];        // relative to the clip's running offsets (see 4. above)
    int last[BM_MAXW], len[BM_MAXW], node[BM_MAXW], par[BM_MAXW], msrc[BM_MAXW];   // par: trie node of the prefix without its last class
    u64 h[BM_MAXW], hp[BM_MAXW];                            // hash of the prefix / of the prefix without its last class
    int nb;
    int lmstate[BM_MAXW];                                   // AUT only: bits 0..22 the prefix's LM state, always in [0, S); bit 31 (BM_LMHELD):
                                                            // nothing to fetch (its rows are already in LDS, or rank without a beam)
};

// VL (ishara_ctc_beam_decode_ex): the clip has Tn = frame_len[b] frames of the buffer's Ts; Ts stays the stride of the logits, of the trie
// workspace and of out_idx (padded with -1 to Ts).  A frame_len[b] outside [1, Ts] is no clip: every n-best slot len -1, score -inf.
template <bool VL, bool AUT>
__global__ __launch_bounds__(BM_MAXNW * WAVE) void ctc_beam_kernel(const float* __restrict__ logits, int Ts, int C, int blank, int W, int nbest,
                                                                  const float* __restrict__ lm, float alpha, float beta,
                                                                  int* __restrict__ ws, int* __restrict__ out_idx, int* __restrict__ out_len,
                                                                  float* __restrict__ out_score, const int* __restrict__ frame_len,
                                                                  const int* __restrict__ lm_next, int nstates, int start_state) {
    __shared__ float s_lm[BM_MAXC * BM_MAXC];               // AUT: rows 0..31 the beams' logp rows, rows 32..63 their next rows (int bits)
    __shared__ float s_lp[BM_CHUNK][BM_MAXC];
    __shared__ BmState s_st[2];
    __shared__ float s_cpnb[BM_MAXW][BM_MAXC];              // pnb' of every candidate (lane b: the same-prefix candidate)
    __shared__ float s_spb[BM_MAXW];                        // pb' of the same-prefix candidates
    __shared__ int s_stamp[BM_MAXW][BM_MAXC];               // == t + 1: extension (i, c) merged into a beam at frame t
    __shared__ u64 s_list[BM_MAXNW][32];
    __shared__ int s_olen[BM_MAXW];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const bool use_lm = lm != nullptr && alpha != 0.0f;
    int Tn = Ts;
    if (VL && frame_len) { Tn = frame_len[b]; if (Tn < 1 || Tn > Ts) Tn = 0; }
    const float* x = logits + (size_t)b * Ts * C;
    int* trie = ws + (size_t)b * ctc_beam_workspace_words(Ts, W);

    if (!AUT && use_lm)
        for (int k = tid; k < C * C; k += blockDim.x) s_lm[(k / C) * BM_MAXC + k % C] = lm[k];
    for (int k = tid; k < BM_MAXW * BM_MAXC; k += blockDim.x) (&s_stamp[0][0])[k] = 0;
    if (tid < BM_MAXW) {
        BmState& s = s_st[0];
        s.pb[tid] = tid == 0 ? 0.0f : BM_NEG;
        s.pnb[tid] = BM_NEG;
        s.bonus[tid] = 0.0f;
        s.last[tid] = -1;
        s.len[tid] = 0;
        s.node[tid] = 0;
        s.par[tid] = 0;
        s.msrc[tid] = -1;
        s.h[tid] = 0;
        s.hp[tid] = 0;
        if (tid == 0) s.nb = 1;
        if constexpr (AUT) {
            s.lmstate[tid] = tid == 0 ? start_state : BM_LMHELD;
        }
    }
    if (tid == 0) trie[0] = 0;
    // wave 0 keeps the clip's offsets and the trie size in registers (every lane the same value)
    double zoff = 0.0, qoff = 0.0;
    int nodes = 1;
    int cur = 0;
    // the logits of a chunk are loaded one chunk ahead (wave w holds frames w, w + NW, ... of it), so their latency overlaps the frames
    const int chunk = min(BM_CHUNK, BM_PRE * nw);
    float pre[BM_PRE];
    auto load_chunk = [&](int t0) {
#pragma unroll
        for (int k = 0; k < BM_PRE; ++k) {
            const int ff = w + k * nw;
            pre[k] = (ff < chunk && t0 + ff < Tn && lane < C) ? x[(size_t)(t0 + ff) * C + lane] : BM_NEG;
        }
    };
    load_chunk(0);
    __syncthreads();

    for (int t = 0; t < Tn; ++t) {
        const int f = t % chunk;
        // AUT: the rows of this wave's beams, issued as soon as the beams are known (the barrier that ended the last frame) and waited
        // for only where they are written to LDS, after 1.  One LDS read per beam stands between that barrier and the loads: the state
        // word says by itself whether to fetch.
        float lm_row[BM_LMPER];
        int lm_nxt[BM_LMPER], lm_st[BM_LMPER];
        if constexpr (AUT) {
            if (use_lm) {
#pragma unroll
                for (int k = 0; k < BM_LMPER; ++k) lm_st[k] = w + k * nw < BM_MAXW ? s_st[cur].lmstate[w + k * nw] : BM_LMHELD;
#pragma unroll
                for (int k = 0; k < BM_LMPER; ++k) {
                    if (lm_st[k] >= 0 && lane < C) {
                        const size_t o = (size_t)lm_st[k] * C + lane;
                        lm_row[k] = lm[o];
                        lm_nxt[k] = lm_next[o];
                    }
                }
            }
        }
        if (f == 0) {                                       // log-softmax of this chunk, one frame per wave at a time
#pragma unroll
            for (int k = 0; k < BM_PRE; ++k) {
                const int ff = w + k * nw;
                if (ff >= chunk || t + ff >= Tn) break;  // uniform per wave
                const float v = pre[k];
                float m = v;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d));
                float e = lane < C ? expf(v - m) : 0.0f;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) e += __shfl_xor(e, d);
                s_lp[ff][lane] = lane < C ? (v - m) - logf(e) : BM_NEG;
            }
            load_chunk(t + chunk);
        }
        BmState& S = s_st[cur];
        BmState& N = s_st[cur ^ 1];
        const int nb = S.nb;
        // 1. merge detection
        for (int q = tid; q < nb * nb; q += blockDim.x) {
            const int i = q / nb, j = q % nb;
            if (S.len[j] == S.len[i] + 1 && S.hp[j] == S.h[i]) {
                int a = S.par[j], c = S.node[i];
                bool eq = true;
                while (a != c) {                            // rare (a re-created prefix); equal lengths: both chains reach the root together
                    const int wa = trie[a], wc = trie[c];
                    if ((wa >> 24) != (wc >> 24)) { eq = false; break; }
                    a = wa & 0xFFFFFF;
                    c = wc & 0xFFFFFF;
                }
                if (eq) {
                    S.msrc[j] = i;
                    s_stamp[i][S.last[j]] = t + 1;
                }
            }
        }
        if constexpr (AUT) {
            if (use_lm) {
#pragma unroll
                for (int k = 0; k < BM_LMPER; ++k) {
                    const int i = w + k * nw;
                    if (lm_st[k] >= 0 && lane < C) {
                        s_lm[i * BM_MAXC + lane] = lm_row[k];
                        s_lm[(BM_MAXW + i) * BM_MAXC + lane] = __int_as_float(lm_nxt[k]);
                    }
                }
            }
        }
        __syncthreads();
        // 2. candidates and the wave's running top-32
        const float lpc = s_lp[f][lane];
        const float lpb = s_lp[f][blank];
        u64 run = 0;
        for (int i = w; i < nb; i += nw) {
            const float pb = S.pb[i], pnb = S.pnb[i], bonus = S.bonus[i];
            const int last = S.last[i];
            const float tot = bm_lse(pb, pnb);
            u64 key = 0;
            if (lane == blank) {
                const float spb = __fadd_rn(tot, lpb);
                float spnb = last >= 0 ? __fadd_rn(pnb, s_lp[f][last]) : BM_NEG;
                const int k = S.msrc[i];
                if (k >= 0) {
                    const float base = S.last[k] == last ? S.pb[k] : bm_lse(S.pb[k], S.pnb[k]);
                    spnb = bm_lse(spnb, __fadd_rn(base, s_lp[f][last]));
                }
                s_spb[i] = spb;
                s_cpnb[i][lane] = spnb;
                const float sc = __fadd_rn(bm_lse(spb, spnb), bonus);
                key = sc > BM_NEG ? bm_key(sc, 0, i, 0) : 0;        // no alignment reaches it: not a candidate
            } else if (lane < C && s_stamp[i][lane] != t + 1) {
                const float epnb = __fadd_rn(lane == last ? pb : tot, lpc);
                const int lmr = AUT ? i : (last >= 0 ? last : blank);      // the LDS row of the beam's LM context
                const float eb = bm_ext_bonus(bonus, use_lm ? s_lm[lmr * BM_MAXC + lane] : 0.0f, alpha, beta, use_lm);
                s_cpnb[i][lane] = epnb;
                const float sc = __fadd_rn(epnb, eb);
                key = sc > BM_NEG ? bm_key(sc, 1, i, lane) : 0;
            }
            key = bm_sort64(key, lane);
            if (i == w) {
                run = lane < 32 ? key : 0;
            } else {
                const u64 rev = bm_shfl(key, 63 - lane);   // the new list's top 32, reversed into lanes 32..63
                run = bm_merge64(lane < 32 ? run : rev, lane);
                if (lane >= 32) run = 0;
            }
        }
        // 3. pairwise merge of the wave lists
        for (int s = nw >> 1; s >= 1; s >>= 1) {
            if (w >= s && w < 2 * s && lane < 32) s_list[w][lane] = run;
            __syncthreads();
            if (w < s) {
                const u64 other = lane >= 32 ? s_list[w + s][63 - lane] : 0;
                run = bm_merge64(lane < 32 ? run : other, lane);
                if (lane >= 32) run = 0;
            }
        }
        if (nw == 1) __syncthreads();                       // no merge round: order the candidate pass's LDS writes before the update
        // 4. new beams (wave 0, lane r = rank r)
        if (w == 0) {
            const bool valid = lane < W && run != 0;
            const uint32_t low = 0xFFFFFFFFu - (uint32_t)run;
            const int kind = (int)(low >> 16), src = (int)((low >> 8) & 0xFF), c = (int)(low & 0xFF);
            float npb = BM_NEG, npnb = BM_NEG, nbonus = 0.0f;
            int nlast = -1, nlen = 0, nnode = 0, npar = 0;
            u64 nh = 0, nhp = 0;
            int nstate = BM_LMHELD;
            if (valid) {
                const int slast = S.last[src];
                const int lmr = AUT ? src : (slast >= 0 ? slast : blank);
                if constexpr (AUT) {
                    if (kind == 0) {
                        nstate = S.lmstate[src] & ~BM_LMHELD;
                        if (src == lane) nstate |= BM_LMHELD;               // same prefix at the same rank: its rows are in place
                    } else if (use_lm) {
                        nstate = __float_as_int(s_lm[(BM_MAXW + src) * BM_MAXC + c]);
                        if ((unsigned)nstate >= (unsigned)nstates) nstate = 0;     // never an index: the table is not readable on the host
                    }
                }
                if (kind == 0) {
                    npb = s_spb[src];
                    npnb = s_cpnb[src][blank];
                    nbonus = S.bonus[src];
                    nlast = slast;
                    nlen = S.len[src];
                    nnode = S.node[src];
                    npar = S.par[src];
                    nh = S.h[src];
                    nhp = S.hp[src];
                } else {
                    npnb = s_cpnb[src][c];
                    nbonus = bm_ext_bonus(S.bonus[src], use_lm ? s_lm[lmr * BM_MAXC + c] : 0.0f, alpha, beta, use_lm);
                    nlast = c;
                    nlen = S.len[src] + 1;
                    npar = S.node[src];
                    nhp = S.h[src];
                    nh = nhp * BM_HASH_MUL + (u64)(c + 1);
                }
            }
            const bool is_ext = valid && kind == 1;
            const u64 eb = __ballot(is_ext);
            if (is_ext) {
                nnode = nodes + __popcll(eb & ((1ull << lane) - 1ull));
                trie[nnode] = S.node[src] | (c << 24);
            }
            nodes += __popcll(eb);
            // renormalise on the top beam (lane 0)
            float dz = __shfl(bm_lse(npb, npnb), 0), dq = __shfl(nbonus, 0);
            if (!(dz > BM_NEG && dz < -BM_NEG)) dz = 0.0f;
            if (!(dq > BM_NEG && dq < -BM_NEG)) dq = 0.0f;
            zoff += (double)dz;
            qoff += (double)dq;
            if (lane < BM_MAXW) {
                N.pb[lane] = __fsub_rn(npb, dz);
                N.pnb[lane] = __fsub_rn(npnb, dz);
                N.bonus[lane] = __fsub_rn(nbonus, dq);
                N.last[lane] = nlast;
                N.len[lane] = nlen;
                N.node[lane] = nnode;
                N.par[lane] = npar;
                N.msrc[lane] = -1;
                N.h[lane] = nh;
                N.hp[lane] = nhp;
                if constexpr (AUT) {
                    N.lmstate[lane] = nstate;
                }
            }
            const int nnb = __popcll(__ballot(valid));
            if (lane == 0) N.nb = nnb;
        }
        cur ^= 1;
        __syncthreads();
    }

    // final ranking: + alpha * lm[last][blank], then (higher score, lower rank); the first nbest go out
    BmState& S = s_st[cur];
    if (w == 0) {
        const int nb = S.nb;
        float fin = BM_NEG;
        u64 key = 0;
        if (lane < nb && !(VL && Tn == 0)) {
            const int last = S.last[lane];
            fin = __fadd_rn(bm_lse(S.pb[lane], S.pnb[lane]), S.bonus[lane]);
            float eos = 0.0f;
            if constexpr (AUT) { if (use_lm) eos = lm[(size_t)(S.lmstate[lane] & ~BM_LMHELD) * C + blank]; }      // the final set's rows were never staged
            else if (use_lm) eos = s_lm[(last >= 0 ? last : blank) * BM_MAXC + blank];
            if (use_lm) fin = __fadd_rn(fin, __fmul_rn(alpha, eos));
            key = ((u64)bm_ord(fin) << 32) | (u64)(0xFFFFFFFFu - (uint32_t)lane);
        }
        key = bm_sort64(key, lane);
        const int r = (int)(0xFFFFFFFFu - (uint32_t)key);
        const float fr = __shfl(fin, key != 0 ? r : 0);
        if (lane < nbest) {
            const size_t o = (size_t)b * nbest + lane;
            if (key != 0) {
                const int len = S.len[r];
                out_len[o] = len;
                out_score[o] = (float)(zoff + qoff + (double)fr);
                s_olen[lane] = len;
                int node = S.node[r];
                int* dst = out_idx + o * Ts;
                for (int k = len - 1; k >= 0; --k) {
                    const int wd = trie[node];
                    dst[k] = wd >> 24;
                    node = wd & 0xFFFFFF;
                }
            } else {
                out_len[o] = -1;
                out_score[o] = BM_NEG;
                s_olen[lane] = 0;
            }
        }
    }
    __syncthreads();
    for (int n = 0; n < nbest; ++n) {
        int* dst = out_idx + ((size_t)b * nbest + n) * Ts;
        for (int k = s_olen[n] + tid; k < Ts; k += blockDim.x) dst[k] = -1;
    }
}

int launch_ctc_beam(const float* logits, int B, int T, int C, int blank, int W, int nbest, const float* lm, float alpha, float beta,
                    void* ws, int* out_idx, int* out_len, float* out_score, hipStream_t s) {
    if (B == 0) return 0;
    int nw = 1;
    while (nw < W && nw < BM_MAXNW) nw <<= 1;
    hipLaunchKernelGGL((ctc_beam_kernel<false, false>), dim3(B), dim3(nw * WAVE), 0, s, logits, T, C, blank, W, nbest, lm, alpha, beta, (int*)ws,
                       out_idx, out_len, out_score, (const int*)nullptr, (const int*)nullptr, 0, 0);
    return launch_rc();
}
int launch_ctc_beam_len(const float* logits, int B, int T, int C, int blank, int W, int nbest, const float* lm, float alpha, float beta,
                        void* ws, int* out_idx, int* out_len, float* out_score, const int* frame_len, hipStream_t s) {
    if (B == 0) return 0;
    int nw = 1;
    while (nw < W && nw < BM_MAXNW) nw <<= 1;
    hipLaunchKernelGGL((ctc_beam_kernel<true, false>), dim3(B), dim3(nw * WAVE), 0, s, logits, T, C, blank, W, nbest, lm, alpha, beta, (int*)ws,
                       out_idx, out_len, out_score, frame_len, (const int*)nullptr, 0, 0);
    return launch_rc();
}
// the automaton LM (AUT): lm_logp / lm_next [S, C]; frame_len may be null (every clip has T frames)
int launch_ctc_beam_lm(const float* logits, int B, int T, int C, int blank, int W, int nbest, const float* lm_logp, const int* lm_next, int S,
                       int start_state, float alpha, float beta, void* ws, int* out_idx, int* out_len, float* out_score, const int* frame_len,
                       hipStream_t s) {
    if (B == 0) return 0;
    int nw = 1;
    while (nw < W && nw < BM_MAXNW) nw <<= 1;
    if (frame_len)
        hipLaunchKernelGGL((ctc_beam_kernel<true, true>), dim3(B), dim3(nw * WAVE), 0, s, logits, T, C, blank, W, nbest, lm_logp, alpha, beta,
                           (int*)ws, out_idx, out_len, out_score, frame_len, lm_next, S, start_state);
    else
        hipLaunchKernelGGL((ctc_beam_kernel<false, true>), dim3(B), dim3(nw * WAVE), 0, s, logits, T, C, blank, W, nbest, lm_logp, alpha, beta,
                           (int*)ws, out_idx, out_len, out_score, (const int*)nullptr, lm_next, S, start_state);
    return launch_rc();
}
