// Edit-operation alignment on the device: the canonical minimal edit script between each clip's decode and its pad-59 target, reduced to
// per-clip operation counts, a per-target-position record and a 60 x 60 confusion matrix summed over the launches (ishara_edit_alignment).
//
// The forward pass is edit_distance_kernel's (score.hip): one wavefront per clip, lane l owns target position j = l + 1, the rows walk the
// prediction, the insertion chain is a shuffle prefix-min.  Once a row's new value D[i][j] is known a lane holds everything that decides its
// cell's first applicable move: diagonal if D[i-1][j-1] + cost == D[i][j], else up if D[i-1][j] + 1 == D[i][j], else left.  Two ballots per
// row (up, left) record the row; lane r keeps the masks of row r of a 64-row chunk and stores them, 16 bytes per lane and coalesced, into
// the workspace ([B, max(T, 11), 2] uint64).  Column 0 has no lane: D[i][0] = i, its move is always up, and the walk knows that.
//
// The walk from (na, nb) to (0, 0) runs with the wave converged on a wave-uniform (i, j).  The masks and prediction symbols of 64 rows are
// held one row per lane (the lane that stored them loads them again: no fence), so no step waits on a global load.  A single wavefront
// issues an instruction every few cycles, so the walk costs steps x instructions: a step takes a whole run of equal moves.  Lane src - k holds
// row i - k, so one ballot of the up-bits of column j gives the up-run below (i, j), one ballot of "neither bit set at column j - k" gives the
// diagonal run, and a left-run is the current row's own left-mask (two readlanes); the run length is a count of leading bits.  Every step
// moves i or j down by at least one and the walk stops at i == 0 (the target positions left are deletions) or j == 0 (the rows left are
// insertions in slot 0), so it ends after at most na + nb steps whatever the masks hold.
//
// Per-clip state stays in registers (lane j-1: the row that took target position j, 0 = deleted; lane j: inserted[j]; slot nb: a uniform
// counter); the aligned symbols are gathered and everything is written once, padding included.  The counts follow: every target position and
// every row is taken exactly once, so D = nb - diagonals and I = na - diagonals.  Confusions go to a per-workgroup LDS histogram in vector
// steps (the diagonal / deletion entries of a clip at its end, the insertions of a chunk when the walk leaves it) and only its non-zero
// entries are added to the matrix: integer atomics, deterministic.
#include "edit_distance.h"

#define SA_NSYM 60                 // the matrix's side: the symbols 0..58 and PAD_TOKEN, its "nothing" row / column
#define SA_WAVES 4

// mask rows per clip: the fallback phrase may be longer than T
__host__ __device__ static inline int sa_rows(int T) { return T > FALLBACK_LEN ? T : FALLBACK_LEN; }
size_t edit_alignment_workspace_bytes(int B, int T) { return (size_t)B * sa_rows(T) * 16; }

// a symbol as a matrix index: anything outside 0..58 is "nothing"
__device__ __forceinline__ int sa_col(int s) { return (unsigned)s < (unsigned)PAD_TOKEN ? s : PAD_TOKEN; }

// the number of consecutive set bits of x from bit p downwards (bit p is set): 1 .. p + 1
__device__ __forceinline__ int sa_run(unsigned long long x, int p) {
    const unsigned long long y = ~x << (63 - p);           // bit p at the top; zeros are shifted in below bit 0, hence the cap
    const int n = y ? (int)__builtin_clzll(y) : 64;
    return n < p + 1 ? n : p + 1;
}

__device__ __forceinline__ void sa_align_clip(const int* __restrict__ out_idx, const int* __restrict__ out_len, int Tn, const int* __restrict__ targets,
                                              int L, int b, int lane, int fallback, int* __restrict__ ops, int* __restrict__ aligned,
                                              int* __restrict__ inserted, int* hist, bool want, ulonglong2* ws) {
    const int j = lane + 1;
    const int bj = lane < L ? targets[(size_t)b * L + lane] : PAD_TOKEN;
    const int nb = __builtin_amdgcn_readfirstlane(target_length(bj));
    int na = out_len[b];
    na = na < 0 ? 0 : (na > Tn ? Tn : na);
    const bool fb = fallback != 0 && na < 3;
    if (fb) na = FALLBACK_LEN;
    na = __builtin_amdgcn_readfirstlane(na);
    const int* a = out_idx + (size_t)b * Tn;
    ulonglong2* rows = ws + (size_t)b * sa_rows(Tn);       // row i of the table at rows[i - 1], i <= na <= sa_rows(Tn)

    // ---- forward: the distance rows, each row's moves as two ballots
    int p = j;                                             // row 0: prev[j] = j
    int a_lane = -1;                                       // after the loop: the last chunk's symbols and masks, one row per lane
    unsigned long long um = 0, lm = 0;
    for (int i0 = 0; i0 < na; i0 += WAVE) {
        const int r_end = na - i0 < WAVE ? na - i0 : WAVE;
        a_lane = lane < r_end ? (fb ? fallback_phrase[i0 + lane] : a[i0 + lane]) : -1;
        um = 0; lm = 0;
        for (int r = 0; r < r_end; ++r) {
            const int i = i0 + r + 1;
            const int ai = __shfl(a_lane, r);
            int left = __shfl_up(p, 1);                    // prev[j-1]
            if (lane == 0) left = i - 1;                   // prev[0]
            const int diag = left + (ai != bj ? 1 : 0);
            int v = min(diag, p + 1) - j;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const int o = __shfl_up(v, d);
                if (lane >= d) v = min(v, o);
            }
            const int pn = j + min(i, v);
            const bool is_diag = diag == pn;
            const bool is_up = !is_diag && p + 1 == pn;
            const unsigned long long u = __ballot(is_up), l = __ballot(!is_diag && !is_up);
            if (lane == r) { um = u; lm = l; }
            p = pn;
        }
        if (lane < r_end) rows[i0 + lane] = make_ulonglong2(um, lm);
    }

    // ---- walk: (i, jj) wave-uniform; the chunk of rows [64 chunk + 1, 64 chunk + 64] is in a_lane / um / lm.  One wavefront issues an
    // instruction every few cycles, so the walk's cost is steps x instructions: a step takes a run of equal moves and records only what
    // cannot be derived later
    int i = na, jj = nb;
    int chunk = na > 0 ? (na - 1) >> 6 : 0;
    int ali = 0;                                           // lane l: the row whose diagonal move took target position l + 1; 0: none, it was deleted
    int ins = 0, ins_row = 0, trail = 0;                   // lane l: inserted[l]; this lane's row of the chunk was an insertion; slot nb
    auto enter_chunk = [&](int c) {                        // c < the last chunk: all of its 64 rows exist
        if (want && ins_row) atomicAdd(&hist[PAD_TOKEN * SA_NSYM + sa_col(a_lane)], 1);
        ins_row = 0;
        const ulonglong2 m = rows[c * WAVE + lane];
        um = m.x; lm = m.y;
        a_lane = fb ? fallback_phrase[c * WAVE + lane] : a[c * WAVE + lane];
        chunk = c;
    };
    while (i > 0 && jj > 0) {
        const int c = (i - 1) >> 6;
        if (c != chunk) enter_chunk(c);
        // a step takes a whole run of equal moves.  From cell (i, jj) the rows below it in the chunk are the lanes below src = (i - 1) & 63:
        // an up-run stays in column jj, a diagonal run has row i - k at column jj - k, a left-run stays in row i
        const int src = (i - 1) & 63, bit = jj - 1;
        const int k = src - lane, col = bit - k;
        const unsigned long long ups = __ballot(((um >> bit) & 1ull) != 0);
        const unsigned long long diags = __ballot(k >= 0 && col >= 0 && (((um | lm) >> (col & 63)) & 1ull) == 0);
        if ((ups >> src) & 1ull) {                         // up: rows i, i-1, .. insert in front of target position jj
            const int n = sa_run(ups, src);
            if (jj == nb) trail += n;
            else if (lane == jj) ins += n;
            if (k >= 0 && k < n) ins_row = 1;
            i -= n;
        } else if ((diags >> src) & 1ull) {                // diagonal: target position jj - k takes row i - k
            const int n = sa_run(diags, src);
            const int t = bit - lane;
            if (t >= 0 && t < n) ali = i - t;
            i -= n; jj -= n;
        } else {                                           // left: this row's left-mask from column jj down
            const unsigned long long row = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(lm >> 32), src) << 32) |
                                           (unsigned)__builtin_amdgcn_readlane((int)lm, src);
            jj -= sa_run(row | (1ull << bit), bit);        // (the bit is set: neither up nor diagonal; or-ed in so that a step always moves)
        }
    }
    // row 0 reached: the target positions left are deletions (their ali stays 0).  Column 0 reached (D[i][0] = D[i-1][0] + 1): the rows
    // left are insertions in slot 0
    if (i > 0) {
        if (nb == 0) trail += i;
        else if (lane == 0) ins += i;
        while (want && i > 0) {                            // their symbols, chunk by chunk
            const int c = (i - 1) >> 6;
            if (c != chunk) enter_chunk(c);
            if (lane <= ((i - 1) & 63)) ins_row = 1;
            i = c * WAVE;
        }
    }

    // ---- outputs, once
    const bool mine = lane < nb;
    const bool hit = mine && ali > 0;
    int sym = -1;
    if (hit) sym = fb ? fallback_phrase[ali - 1] : a[ali - 1];             // ali <= na
    const int n_diag = (int)__popcll(__ballot(hit)), n_match = (int)__popcll(__ballot(hit && sym == bj));
    const int n_del = nb - n_diag, n_ins = na - n_diag;                // every target position and every row is taken exactly once
    if (want) {
        if (ins_row) atomicAdd(&hist[PAD_TOKEN * SA_NSYM + sa_col(a_lane)], 1);
        if (mine) atomicAdd(&hist[sa_col(bj) * SA_NSYM + (hit ? sa_col(sym) : PAD_TOKEN)], 1);
    }
    if (lane < 4) ops[(size_t)b * 4 + lane] = lane == 0 ? n_match : (lane == 1 ? n_diag - n_match : (lane == 2 ? n_del : n_ins));
    if (lane < L) aligned[(size_t)b * L + lane] = mine ? (hit ? sym : -1) : -2;
    int* ins_out = inserted + (size_t)b * (L + 1);
    if (lane <= L) ins_out[lane] = lane < nb ? ins : (lane == nb ? trail : 0);
    if (L == WAVE && lane == 0) ins_out[WAVE] = nb == WAVE ? trail : 0;      // slot 64 has no lane
}

__global__ __launch_bounds__(SA_WAVES * WAVE) void edit_alignment_kernel(const int* __restrict__ out_idx, const int* __restrict__ out_len, int Tn,
                                                                         const int* __restrict__ targets, int L, int B, int fallback,
                                                                         int* __restrict__ ops, int* __restrict__ aligned, int* __restrict__ inserted,
                                                                         int* confusion, ulonglong2* ws) {
    __shared__ int hist[SA_NSYM * SA_NSYM];
    const bool want = confusion != nullptr;                // uniform over the grid
    if (want) {
        for (int k = threadIdx.x; k < SA_NSYM * SA_NSYM; k += SA_WAVES * WAVE) hist[k] = 0;
        __syncthreads();
    }
    const int b = blockIdx.x * SA_WAVES + (threadIdx.x >> 6);
    if (b < B)                                             // uniform per wave; the waves past B only share the histogram's barriers
        sa_align_clip(out_idx, out_len, Tn, targets, L, b, threadIdx.x & 63, fallback, ops, aligned, inserted, hist, want, ws);
    if (want) {
        __syncthreads();
        for (int k = threadIdx.x; k < SA_NSYM * SA_NSYM; k += SA_WAVES * WAVE) {
            const int n = hist[k];
            if (n) atomicAdd(&confusion[k], n);
        }
    }
}

int launch_edit_alignment(const int* out_idx, const int* out_len, int B, int T, const int* targets, int L, int fallback, int* ops, int* aligned,
                          int* inserted, int* confusion, void* ws, hipStream_t s) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(edit_alignment_kernel, dim3((B + SA_WAVES - 1) / SA_WAVES), dim3(SA_WAVES * WAVE), 0, s, out_idx, out_len, T, targets, L, B,
                       fallback, ops, aligned, inserted, confusion, (ulonglong2*)ws);
    return launch_rc();
}
