// Kernel launchers of the ishara_amd HIP library.  Host-callable; every launch is
// asynchronous on the given stream, allocates nothing and never synchronises.
#pragma once
#include "common.h"
#include "../../include/ishara_hip.h"

enum DType : int { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };       // DT_F16: forward (inference) kernels only
static inline size_t dt_size(int dt) { return dt == DT_F32 ? 4 : 2; }
static inline bool dt_is16(int dt) { return dt != DT_F32; }
// the byte ranges [a, a + na) and [b, b + nb) share a byte (the launchers' refusals); a NULL buffer overlaps nothing
static inline bool bytes_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + nb && b0 < a0 + na;
}

// ---- operand transforms applied while staging a GEMM operand -------------------
enum : int { OP_NONE = 0, OP_SWISH = 1, OP_COLAFFINE = 2, OP_ROWSCALE = 3, OP_DROPMASK = 4 };
struct OpArgs {
    const float* c1 = nullptr;   // OP_COLAFFINE: v*c1[col]+c0[col]
    const float* c0 = nullptr;
    const float* rs = nullptr;   // OP_ROWSCALE: v*rs[row / T]
    int T = 1;
    DropSpec drop = {0, 0, 1.f}; // OP_DROPMASK: v*mask(row, col)
};

// ---- GEMM epilogue (NT kernel) ---------------------------------------------------
enum : int { ACT_NONE = 0, ACT_SWISH = 1, ACT_RELU = 2 };
enum : int { DACT_NONE = 0, DACT_SWISH = 1, DACT_POS = 2 };
enum : int { EPI_STD = 0, EPI_QKV = 1 };
struct EpiArgs {
    const float* bias = nullptr;      // [N]
    const float* addtab = nullptr;    // += addtab[(m % tab_period)*N + n]
    int tab_period = 1;
    void* pre_out = nullptr;          // save pre-activation (TC, [M,N])
    int act = ACT_NONE;
    DropSpec drop = {0, 0, 1.f};      // elementwise inverted dropout (row=m, col=n)
    const float* rowscale = nullptr;  // *= rowscale[m / T]
    int T = 1;
    int rowscale_bias = 0;            // 1: the row scale multiplies the BIAS only (the A operand already carries it): acc + bias * rowscale[m / T]
    int dact = DACT_NONE;             // *= act'(aux[m,n])
    const void* aux = nullptr;        // TC, [M,N]
    const void* resid = nullptr;      // TC, [M,N]
    int mode = EPI_STD;               // EPI_QKV: scatter to q,k [B,H,T,dh] and vt [B,H,dh,T]
    void* q = nullptr; void* k = nullptr; void* vt = nullptr;
    int H = 1, dh = 1;
    int dbg = 0;                      // ablation bits (tools/gemm_ablate.py): 1 skip epilogue, 2 skip MFMA, 4 skip loads
    // ---- prologues of the A-stationary kernel (gemm_as.hip): the operand rows are transformed in registers after the load, and the
    // transformed rows are written out once (the weight-gradient GEMM of the backward pass needs them in memory)
    const float* ln_gamma = nullptr;  // LayerNorm over K (the wave holds whole rows): A' = (A - mean) * rstd * gamma + beta
    const float* ln_beta = nullptr;
    float ln_eps = 0.f;
    float* ln_mean = nullptr;         // [M] row statistics for the LayerNorm backward (may be null)
    float* ln_rstd = nullptr;
    const float* pa_P = nullptr;      // per-sample affine: A' = A * pa_P[m / T, k] + pa_Q[m / T, k]   (BatchNorm + ECA gate of a Conv1DBlock)
    const float* pa_Q = nullptr;
    void* pro_out = nullptr;          // A' rows [M, K] in the operand type (null: not needed, inference)
    int head_major = 1;               // 1: cols = h*3dh + {q,k,v}*dh + i (TF path); 0: {q,k,v}*d + h*dh + i (torch twin)
    // A-stationary kernel only: C rows are ldc elements apart (0: N) and only the columns below n_valid are stored (0: all) — a 60-column
    // classifier runs as N = 64 over the zero-padded weight shadow (no residual / act' operands with these)
    int ldc = 0, n_valid = 0;
    // A-stationary kernel, 16-bit C: bit 0 — a row's two 64-byte halves of a 128-byte line are stored back to back every second column step
    // instead of one step apart (cold HBM takes half lines that arrive a step apart at 3.8 TB/s, whole lines at 4.6+: tools/micro/store_cold.hip);
    // bit 1 — non-temporal hint on the side outputs (saved pre-activations, prologue rows); bits 4 / 5 — the chunked form (one workgroup per CU, 64 KB
    // weight stages, a wait + barrier per stage instead of per column step) at K = 256 / 512; bit 6 — the C-stationary kernel (gemm_cs.hip) for K = 512, N = 256 at
    // M > 49152, bit 7 — at any M (tests).  -1: the library default (115; ISHARA_AS_FLAGS)
    int as_flags = -1;
};

// C[M,N] = epi( op(A)[M,K] . Bt[N,K]^T ).  Bt is a padded weight shadow: rows padded to
// a multiple of 128, row stride ldb (elements) a multiple of the K tile (64 bf16 / 32 f32).
int launch_gemm_nt(int dtA, int dtM, int dtC, int op, const void* A, const void* Bt, void* C,
                   int M, int N, int K, int ldb, const OpArgs& oa, const EpiArgs& ea, hipStream_t s);
// the kernel launch_gemm_nt runs a call on (gemm_nt.hip: the one place that decides), and its profiler key = the prefix of its rocprof name
enum NtRoute { NT_REFUSED, NT_AS_F16, NT_BIG, NT_CS, NT_AS, NT_TILE_T, NT_GLDS, NT_REG };
NtRoute gemm_nt_route(int dtA, int dtM, int dtC, int op, const void* A, int M, int N, int K, int ldb, const EpiArgs& ea);
const char* gemm_nt_kernel_name(int dtA, int dtM, int dtC, int op, const void* A, int M, int N, int K, int ldb, const EpiArgs& ea);
bool gemm_nt_as_applicable(int dtC, int M, int N, int K, int ldb, const EpiArgs& ea);                    // gemm_as.hip
// the kernel also takes ea's prologue (ln_* / pa_*): bf16 output, K in {256, 512}, whole 16-row tiles inside one sample for pa_*
bool gemm_nt_as_prologue_ok(int dtA, int dtM, int dtC, int M, int N, int K, int ldb, const EpiArgs& ea);   // gemm_as.hip: the A-stationary kernel takes this shape
const char* gemm_nt_as_name(int dtC, int K, const EpiArgs& ea, int M, int N);
// what the A-stationary launcher does with a call (gemm_as.hip: the one place that decides; run_as launches from it, gemm_nt_as_prologue_ok,
// gemm_nt_as_name and ishara_debug_gemm_as_plan read it).  rows / gx: rows per workgroup and workgroups along M of the kernel that runs (the chunked
// one: 384); plain_rows / plain_gx: the same for the per-step kernel; gy: column splits; nsteps: 32-column steps per workgroup; ring: weight stages
// in LDS; cs: column steps per stage; passes / pass_rows: the sequential row passes of a workgroup; hold: paired stores; inst: the compiled
// epilogue mask (255: every feature behind its run-time flag; -1: none for this prologue); pro: 0 none, 1 LayerNorm, 2 per-sample affine.  Host only
struct AsPlan { int rows, gx, plain_rows, plain_gx, gy, nsteps, ring, cs, waves, passes, pass_rows[2], chunked, hold, inst, pro; };
bool gemm_nt_as_plan(int dtM, int dtC, int M, int N, int K, const EpiArgs& ea, AsPlan* p);
int gemm_nt_as_mask(const EpiArgs& ea);      // the epilogue feature mask of a call (bits: gemm_as.hip AS_RESID ..)
int launch_gemm_nt_as(int dtC, const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea, hipStream_t s);
int launch_gemm_nt_as_f16(int dtC, const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea, hipStream_t s);   // gemm_as_f16.hip
// the C-stationary kernel of the K = 512 -> N = 256 projections and the K = 768 -> N = 256 plain dgrad at training-size M (gemm_cs.hip; as_flags bit 6 turns
// the route on, bit 7 drops the row threshold, bit 8 keeps K = 768 on the tile kernel)
bool gemm_nt_cs_applicable(int dtC, int M, int N, int K, int ldb, const EpiArgs& ea);
const char* gemm_nt_cs_name(int K, const EpiArgs& ea);
int launch_gemm_nt_cs(int dtC, const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea, hipStream_t s);
bool gemm_nt_big_applicable(int dtA, int dtM, int dtC, int op, const void* A, int M, int N, int K, int ldb, const EpiArgs& ea);              // gemm_big.hip
int launch_gemm_nt_big(int dtA, int dtM, int dtC, int op, const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea, hipStream_t s);

// dW[Ka,Nb] += opA(A)[M,Ka]^T . opB(B)[M,Nb]   (fp32 accumulate into `out`, row-major [Ka,Nb]);
// dbias[Nb] += colsum(opB(B)) when dbias != nullptr.  slab = fp32 scratch of
// gemm_tn_slab_floats(...) floats.
size_t gemm_tn_slab_floats(int M, int Ka, int Nb, int dtM);
// ---- batched, deferred column sums of partial rows (parameter gradients of LayerNorm / depthwise conv: ~45 launches of ~5 us per step, all off
// the backward pass's dependency chain).  While a RedSink is installed (g_red_sink), launch_reduce_slabs / _slabs2 record the job instead of
// launching; the caller keeps every recorded slab intact (a bump arena) until launch_reduce_flush sums all of them in ONE launch, each output element in a fixed
// order (run-to-run bit-identical gradients; not the same order as the single launches).
#define RED_MAXJOBS 48
struct RedJob { const float* slab; float* out0; float* out1; size_t stride; int n0, n, splits, nb, nbv, first_block; };
struct RedSink { RedJob job[RED_MAXJOBS]; int njobs = 0; int nblocks = 0; };
extern RedSink* g_red_sink;
// out[0..n) += column sums of slab[:, 0..n) (rows `stride` floats apart); _slabs2: out0[0..n0) and out1[0..n1) from slab[:, 0..n0) and [n0..n0+n1) in one launch
void launch_reduce_slabs(const float* slab, float* out, int n, int splits, size_t stride, hipStream_t s);
void launch_reduce_slabs2(const float* slab, float* out0, int n0, float* out1, int n1, int splits, size_t stride, hipStream_t s, int nb = 0, int nbv = 0);
bool reduce_cols_ok(const float* slab, const float* out0, const float* out1, int n0, int n, size_t stride);   // the atomics-free column kernels (and a RedSink) take the job
bool reduce_sink_full();                                   // no room for another job: flush before the next deferring operator
int launch_reduce_flush(RedSink* sink, hipStream_t s);
bool gemm_tn_bias_rowscale_ok(int dtA, int dtB, int dtM, int M, int Ka, int Nb, int T);   // the transposed-read kernel takes the call and T % 32 == 0
// Deferred slab sums of the transposed-read wgrad kernel: with a TnDefer the launch writes slab[turn] (two caller-owned buffers of
// gemm_tn_slab_floats floats each) and the sums of ITS slabs are carried by the next deferring launch as extra workgroups;
// launch_gemm_tn_flush sums what is still pending.  Launches that take another kernel ignore it (their sums run at once on `slab`).
struct TnDefer { float* slab[2] = {nullptr, nullptr}; int turn = 0; bool pending = false;
                 const float* p_slab = nullptr; float* p_out0 = nullptr; float* p_out1 = nullptr; int p_n0 = 0, p_n = 0, p_splits = 0; size_t p_stride = 0; int p_nb = 0, p_nbv = 0; };
int launch_gemm_tn_flush(TnDefer* defer, hipStream_t s);
// Per-sample affine of the A operand inside the transposed-read wgrad kernel (the project conv of a Conv1DBlock, c5:41-89): the operand the
// forward pass multiplied was A'[m,k] = A[m,k] * P[b,k] + Q[b,k] (BatchNorm . ECA gate . drop-path, b = m / T), but only A is in memory.
// The kernel accumulates A_b^T B_b per sample, folds it into the total with P[b,:] (and Q[b,:] x the sample's column sums of B) at every
// sample boundary, and from the same per-sample accumulator emits what the BatchNorm / ECA backward needs from the gradient of A'
// (dA' = rs[b] * B W^T, never read back): Rpart[b][p][k] = sum over the 64-column group p of W[k,n] * (A_b^T B_b)[k,n], i.e. partial
// sums of sum_t dA'[b,t,k] * A[b,t,k] / rs[b], and G[b,n] = sum_t B[b,t,n].
struct TnPsa { const float* P = nullptr; const float* Q = nullptr;     // [B, Ka]
               const void* W = nullptr; int ldw = 0;                     // bf16 [Ka][ldw]: the dgrad's weight shadow
               float* G = nullptr; float* Rpart = nullptr; int T = 0;     // [B, Nb], [B][Nb / 64][Ka]
               int dbg = 0; };                                           // timing ablation (ISHARA_PSA_DBG; results are wrong): 1 no per-sample work, 2 no column sums, 4 no setup loads, 16 no write-out
bool gemm_tn_psa_ok(int dtA, int dtB, int dtM, int M, int Ka, int Nb, int T);
int launch_gemm_tn(int dtA, int dtB, int dtM, int opA, int opB, const void* A, const void* B,
                   float* out, float* dbias, float* slab, int M, int Ka, int Nb,
                   const OpArgs& oa, const OpArgs& ob, hipStream_t s, int ka_valid = 0, int nb_valid = 0,
                   const float* bias_rowscale = nullptr, int bias_T = 0, TnDefer* defer = nullptr, const TnPsa* psa = nullptr);   // bias_rowscale: dbias = sum_m bias_rowscale[m / bias_T] * B[m,:] (gemm_tn_bias_rowscale_ok shapes only); ka_valid < Ka: A columns [ka_valid, Ka) are zero padding, out has ka_valid rows; nb_valid < Nb: same for B / out columns / dbias
// C[M, N] (f32) = A[M, K] (bf16 / fp16) . Wt[N, K]^T + bias for a NARROW output (N <= 64: the classifier) and few rows: a lane per output
// column, four rows per wave, the weight row streamed from L2 — the 64 x 128 tile kernel needs 37 us for M = 384, N = 60, K = 512
// (6 workgroups); this one is for the latency of a B = 1 clip, not for throughput (M <= 4096)
int launch_dense_narrow(int dt, const void* A, const void* Wt, int ldt, const float* bias, float* C, int M, int N, int K, hipStream_t s);
// xb[M, Kp] (bf16) = x[M, F] (f32), zero padded to Kp columns (F % 4 == 0, Kp % 8 == 0)
int launch_pack_rows_bf16(const float* x, void* xb, int M, int F, int Kp, hipStream_t s, int dt = DT_BF16);   // dt: DT_BF16 or DT_F16 (the fp16 inference path)

// the kernel launch_gemm_tn runs a call on (gemm_tn.hip: the one place that decides; arguments as the launcher's, brs / psa: there is a bias row scale / a TnPsa)
enum TnRoute { TN_REFUSED, TN_BIG, TN_TR, TN_TR_BRS, TN_TR_PSA, TN_REG };
TnRoute gemm_tn_route(int dtA, int dtB, int dtM, int opA, int opB, int M, int Ka, int Nb, int ka_valid, int nb_valid, bool brs, int brsT, bool psa, int psaT);
const char* gemm_tn_kernel_name(int dtA, int dtB, int dtM, int opA, int opB, int M, int Ka, int Nb, int ka_valid = 0, int nb_valid = 0,
                                const float* bias_rowscale = nullptr, int bias_T = 0, const TnPsa* psa = nullptr);
// what launch_gemm_tn does with a call: the route (TN_REFUSED: the launcher's message is set) and the split plan it launches with — M-splits and
// rows per split.  launch_gemm_tn launches from this and ishara_debug_gemm_tn_plan reports it.  Host only; A / B: alignment only, nothing is read
struct TnPlan { TnRoute route; int splits, rps; };
TnPlan gemm_tn_plan(int dtA, int dtB, int dtM, int opA, int opB, const void* A, const void* B, bool has_dbias, int M, int Ka, int Nb,
                    int ka_valid, int nb_valid, const float* bias_rowscale, int bias_T, const TnPsa* psa);
// the 256 x 256 tile wgrad kernel (gemm_big.hip): rows per M-split (0: not a shape it takes); the launcher answers 1 for such a shape
int gemm_tn_big_plan(int M, int Ka, int Nb, int* splits_out);
int launch_gemm_tn_big(const void* A, const void* B, float* slab, int want_bias, int M, int Ka, int Nb, int* splits_out, const float* brs, int brsT, hipStream_t s);
extern int g_force_tn_regstage;   // tests: 1 forces the register-transposing TN kernel
// the other switches of ishara_debug_force_regstage / _set_as_flags / _set_nt_big (api_ops.hip sets them; defined beside the kernels they steer)
extern int g_force_regstage, g_dbg_tn, g_force_dw_lds, g_tn_blocks, g_attn_bwd_two_pass, g_as_flags_override, g_nt_big;
extern int g_tn_phase;   // 0 GEMM + slab sums, 1 GEMM kernel only, 2 slab sums only

// weight shadows: Wt[Np][Kp] (transposed) and Wn[Kp2][Np2] (as-is, padded) in dtM
int launch_make_shadow(int dtM, const float* W, int K, int N, void* Wt, int ldt, void* Wn, int ldn, hipStream_t s);
struct ShadowDesc { const float* W; void* Wt; void* Wn; int K, N, ldt, ldn, tile0, tiles_n; };   // tile0: first 32x32 tile (block) of this weight
int launch_make_shadow_batched(int dtM, const ShadowDesc* tab, int ntab, int total_tiles, hipStream_t s);

// ---- row-wise passes: log-softmax, LayerNorm (norm_rows.hip; launch_map_rows is declared further down) ------------
int launch_log_softmax_fwd(const float* x, float* y, int M, int C, int ld, hipStream_t s);
int launch_log_softmax_bwd(const float* dy, const float* y, float* dx, int M, int C, int ld, hipStream_t s);
int launch_layernorm_fwd(int dt, const void* x, const float* gamma, const float* beta, float eps,
                         void* y, float* mean, float* rstd, int M, int C, hipStream_t s);
// dx = LN'(dy) (+ resid) ; dgamma/dbeta += column sums: through per-block partial rows in `scratch`
// (layernorm_bwd_scratch_floats(C) floats) + a slab reduce, or same-address atomics if scratch == nullptr
size_t layernorm_bwd_scratch_floats(int C);
int launch_layernorm_bwd(int dt, const void* dy, const void* x, const float* mean, const float* rstd,
                         const float* gamma, const void* resid, void* dx, float* dgamma, float* dbeta,
                         float* scratch, int M, int C, hipStream_t s);

// ---- depthwise conv (dwconv.hip: forward kernels, routes, launchers; dwconv_bwd.hip: one-pass backward, weight gradients) ------------
enum : int { DWIN_NONE = 0, DWIN_SWISH = 1, DWIN_GLU = 2 };
#define DW_CT 128          // channels per workgroup of the LDS-tiled kernels
#define DW_MAXK 31         // largest kernel size
#define DWG_BLOCKS 512     // most partial rows a backward kernel writes: dwconv_bwd_scratch_floats (the model sizes its arenas by it)
// y[b,t,c] = bias[c] + sum_j w[j,c] * in(x)[b, t - padl + j, c]; x has Cin = C (or 2C for GLU).
// stats: ssum/ssq [B,C] = per-sample sum_t y, sum_t y^2 (fp32 atomics; zero them first; nullptr = off).
// ssum / ssq: per-sample channel sums of y and y^2 [B, C] (or nullptr).  `part`: scratch of dwconv_fwd_scratch_floats(B, T, C)
// floats -> deterministic sums without atomics or zero fills; nullptr -> the caller zero-fills ssum / ssq, float atomics
int launch_dwconv_fwd(int dt, int inop, const void* x, const float* w, const float* bias, void* y,
                      float* ssum, float* ssq, float* part, int B, int T, int C, int k, int padl, hipStream_t s, int* part_rows = nullptr);
// part_rows != nullptr: the partial statistic rows stay unsummed in `part` ([B][rows][2][C]: sum | sum of squares), *part_rows = rows per sample
size_t dwconv_fwd_scratch_floats(int B, int T, int C);
// dx = d in(x) ; dw [k,C], dbias [C] accumulated (through `scratch` partial rows of
// dwconv_bwd_scratch_floats(C,k) floats when given, else atomically).
size_t dwconv_bwd_scratch_floats(int C, int k);
// BatchNorm backward folded into the depthwise-conv backward: dy is the gradient of BN(y), h = y (the conv's forward output, [B,T,C]);
// the kernel applies dy <- a[c] * (dy*sg[b,c] + E[b or 0,c] - xhat*Fc[c]) (the arithmetic of launch_bn_bwd_apply) to each dy row as it
// loads it.  h == nullptr: plain depthwise-conv backward.
struct DwBnArgs { const void* h = nullptr; const float* mean = nullptr; const float* rstd = nullptr; const float* a = nullptr;
                  const float* sg = nullptr; const float* E = nullptr; const float* Fc = nullptr; int e_per_sample = 0; };
// returns 1 when the fused one-pass kernel took the call (dx, dw, dbias written), 0 when this shape has no fused kernel (the caller
// runs launch_bn_bwd_apply + launch_dwconv_bwd instead), < 0 on error
int launch_dwconv_bwd_bn(int dt, int inop, const void* dy, const DwBnArgs& bn, const void* x, const float* w, void* dx,
                         float* dw, float* dbias, float* scratch, int B, int T, int C, int k, int padl, hipStream_t s);
int launch_dwconv_bwd(int dt, int inop, const void* dy, const void* x, const float* w, void* dx,
                      float* dw, float* dbias, float* scratch, int B, int T, int C, int k, int padl, hipStream_t s);
// The kernel a call runs on (dwconv.hip: the one place that decides and that reads g_force_dw_lds / ISHARA_NO_DW_STREAM); the launchers
// and the name functions are switches over it.  stats: ssum is wanted; part / scratch: the caller gave the scratch; bn: DwBnArgs.h is set
enum DwFwdRoute { DWF_REFUSED, DWF_STREAM, DWF_REG8, DWF_REG, DWF_TILE };
DwFwdRoute dwconv_fwd_route(int dt, int B, int T, int C, int k, bool stats, bool part);
int dwconv_fwd_part_rows(DwFwdRoute route, int B, int T, int C, int* tsplit = nullptr);      // partial statistic rows per sample that route's kernel writes
enum DwBwdKind { DWB_REFUSED, DWB_FUSED_BN, DWB_FUSED, DWB_TWO_PASS };      // FUSED_BN only when bn was asked for; otherwise what launch_dwconv_bwd runs
enum DwDgrad { DWD_REG, DWD_TILE };
enum DwWgrad { DWW_WIN, DWW_TILE_PART, DWW_TILE_ATOMIC };
struct DwBwdRoute { DwBwdKind kind; DwDgrad dgrad; DwWgrad wgrad; };         // dgrad, wgrad: the two kernels of DWB_TWO_PASS
DwBwdRoute dwconv_bwd_route(int dt, int C, int k, int padl, bool scratch, bool bn);
// the prefix of the kernel's rocprof name ("" when refused; a two-pass backward as "dgrad+wgrad")
const char* dwconv_fwd_kernel_name(int dt, int B, int T, int C, int k, bool stats, bool part);
const char* dwconv_bwd_kernel_name(int dt, int C, int k, int padl, bool scratch, bool bn);
// the kernels of dwconv_bwd.hip behind the two backward launchers.  The one-pass kernel: partial rows into `part`, summed by the caller
int launch_dwconv_bwd_fused(int dt, int inop, const void* dy, const void* x, const float* w, void* dx, float* part,
                            int B, int T, int C, int k, int padl, int max_rows, hipStream_t s, const DwBnArgs& bn);
// the weight gradient of the two-pass backward (kind: which kernel; DWW_WIN takes k in {3, 5, 11, 15}): the partial rows written to `part`, 0 with part == nullptr (atomics into dw / dbias)
int launch_dwconv_wgrad(DwWgrad kind, int dt, int inop, const void* dy, const void* x, float* dw, float* dbias, float* part, int B, int T, int C, int k, int padl, hipStream_t s);

// ---- BatchNorm / ECA / Squeeze-Excite and the passes that apply them (bn_gate.hip) ---------------------------------
// BN finalize from per-sample sums ssum/ssq [nb,C] (count = rows they cover): mean, rstd,
// a = gamma*rstd, b = beta - mean*a ; moving statistics update when training
int launch_bn_finalize(const float* ssum, const float* ssq, int nb, float count, const float* gamma, const float* beta,
                       float eps, float momentum, float* moving_mean, float* moving_var, int training,
                       float* mean, float* rstd, float* a, float* b, int C, hipStream_t s, float var_corr = 1.f, int stride = 0);   // var_corr: factor on the batch variance
                                                                                                                       // entering moving_var (torch: n/(n-1)); stride: floats between rows of ssum / ssq (0: C)
// ECA fwd on [B,C]: g = a*gap/T + b ; s = sigmoid(conv5(g)) ; P = a*s ; Q = b*s
int launch_eca_fwd(const float* gap, const float* a, const float* b, const float* w5, float invT,
                   float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s, float* rs = nullptr, DropSpec dp = {0, 0, 1.f}, int dp_fold = 0);
// rs != nullptr: the kernel also draws the per-sample drop-path scale rs[b] (dp) and, with dp_fold, scales P and Q by it
// training form over the depthwise conv's partial statistic rows part[B][prows][2][C] (no stats_reduce launch): per-sample sums -> gap_out [B, C]
int launch_eca_fwd_part(const float* part, int prows, float* gap_out, const float* a, const float* b, const float* w5, float invT,
                        float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s, float* rs = nullptr, DropSpec dp = {0, 0, 1.f}, int dp_fold = 0);
// inference form: the sample's channel sums come from the depthwise conv's partial rows, a / b from the BatchNorm's moving statistics
int launch_eca_fwd_infer(const float* part, int prows, const float* mm, const float* mv, const float* gamma, const float* beta, float eps, const float* w5, float invT,
                         float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s);
// y = x*P[b,c] + Q[b,c] (+ resid)    (P,Q per sample) ; if Q == nullptr -> no offset
int launch_sample_affine(int dt, const void* x, const float* P, const float* Q, const void* resid, void* y,
                         int B, int T, int C, hipStream_t s);
// y = x*a[c] + b[c]
int launch_col_affine(int dt, const void* x, const float* a, const float* b, void* y, int M, int C, hipStream_t s);
enum : int { MAP_SWISH = 0, MAP_ROWSCALE = 1, MAP_DROPMASK = 2 };
// y = swish(x) | x * rs[row / T] | x * dropmask(row, col)   — one streaming pass over [M, C] (norm_rows.hip)
int launch_map_rows(int dt, int op, const void* x, void* y, const float* rs, DropSpec drop, int M, int T, int C, hipStream_t s);
// per-sample reductions over t: S1[b,c] = sum_t dy ; S2[b,c] = sum_t dy * other   (other optional,
// normalised as (other-mean[c])*rstd[c] when mean != nullptr)
int launch_sample_reduce(int dt, const void* dy, const void* other, const float* mean, const float* rstd,
                         float* S1, float* S2, int B, int T, int C, hipStream_t s);
// Conv1DBlock BN+ECA backward finalize (one block; small)
// PsaStats: S1, S2 are not inputs but computed first, per sample, from what the per-sample-affine weight-gradient GEMM emitted (TnPsa):
// S1[b,c] = rs[b] * sum_n Wt[n,c] G[b,n] (= sum_t dh4[b,t,c]), S2[b,c] = rstd[c] * (rs[b] * sum_p Rpart[b][p][c] - mean[c] * S1[b,c]); Wt = bf16 [N][ldt]
#define ECA_MAX_CHUNKS 4          // eca_bwd_sample_kernel splits the channels of a sample over up to 4 workgroups: dw5part holds B * 4 * 8 floats
struct PsaStats { const float* G = nullptr; const float* Rpart = nullptr; int nparts = 0; const void* Wt = nullptr; int ldt = 0, N = 0;
                  const float* rs = nullptr; const float* mean = nullptr; const float* rstd = nullptr; };
int launch_eca_bn_bwd_finalize(float* S1, float* S2, const float* gap, const float* gn, const float* sgate,
                               const float* w5, const float* gamma, const float* beta, const float* mean, const float* rstd,
                               float* dgamma, float* dbeta, float* dw5, float* E, float* Fc, float* dw5part /* B * ECA_MAX_CHUNKS * 8 floats */, int B, int T, int C, hipStream_t s,
                               const PsaStats* ps = nullptr, const int* frame_len = nullptr, float* Ecol = nullptr);
// frame_len != nullptr (no PsaStats): `gap` is the masked mean of launch_masked_time_mean; E[b,c] = dgn / n_b is for the frames t < n_b only and
// Ecol[c] = -dbeta / Mtot for every frame: launch_bn_bwd_apply_len applies them
// plain BN backward finalize from per-sample S1,S2: dgamma, dbeta, E[c] = -dbeta/Mtot, Fc = dgamma/Mtot
int launch_bn_bwd_finalize(const float* S1, const float* S2, float* dgamma, float* dbeta, float* Ecol, float* Fc,
                           int B, int T, int C, hipStream_t s);
// dx = a[c] * (dy*sg[b,c] + E[b or 0,c] - xhat*Fc[c]) ; sg optional ; E per-sample if e_per_sample
int launch_bn_bwd_apply(int dt, const void* dy, const void* x, const float* mean, const float* rstd, const float* a,
                        const float* sg, const float* E, int e_per_sample, const float* Fc, void* dx,
                        int B, int T, int C, hipStream_t s);
// Squeeze-Excite MLP on [B,C]: z = gap/T ; h = swish(z W1 + b1) ; se = sigmoid(h W2 + b2)
int launch_se_fwd(const float* gap, float invT, const float* W1, const float* b1, const float* W2, const float* b2,
                  float* hid_pre, float* se, int B, int C, int R, hipStream_t s);
// given dse[b,c] (= sum_t dOut*u3): grads of W1,b1,W2,b2 (atomic) and dgapT[b,c] = dL/dgap * (1/T)
int launch_se_bwd(const float* dse, const float* gap, float invT, const float* W1, const float* W2,
                  const float* hid_pre, const float* se, float* dW1, float* db1, float* dW2, float* db2,
                  float* dgapT, float* scr /* B*(C+2R) floats */, int B, int C, int R, hipStream_t s);

// ---- per-clip frame lengths of the Keras hybrid family (frame_mask.hip): frame_len [B] int32 on the device, clamped to [0, T] in the kernels;
// clip b has n_b = frame_len[b] real frames, the rest is padding.  Kernels of their own: the unmasked ones above are not touched
// out[b,c] = (sum_{t < n_b} x[b,t,c]) / n_b, 0 at n_b = 0; rows t >= n_b are not read.  The Squeeze-Excite kernels above then run with invT = 1
int launch_masked_time_mean(int dt, const void* x, const int* frame_len, float* out, int B, int T, int C, hipStream_t s);
// ECA fwd on [B,C] from the masked mean: g = a*mean + b (0 at n_b = 0: nothing to pool); s, P, Q and the drop-path draw as launch_eca_fwd
int launch_eca_fwd_len(const float* mean, const float* a, const float* b, const float* w5, const int* frame_len, int T,
                       float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s, float* rs = nullptr, DropSpec dp = {0, 0, 1.f}, int dp_fold = 0);
// dx = a[c] * (dy*sg[b,c] + [t < n_b] Ev[b,c] + Ecol[c] - xhat*Fc[c])
int launch_bn_bwd_apply_len(int dt, const void* dy, const void* x, const float* mean, const float* rstd, const float* a, const float* sg,
                            const float* Ev, const float* Ecol, const float* Fc, const int* frame_len, void* dx, int B, int T, int C, hipStream_t s);
// y = x*P[b,c] + [t < n_b] Q[b,c] / n_b
int launch_sample_affine_len(int dt, const void* x, const float* P, const float* Q, const int* frame_len, void* y, int B, int T, int C, hipStream_t s);
// out_len[b] = 1 + index of the last frame of x [B,T,F] with a non-zero feature (0: none)
int launch_frame_lengths(const float* x, int B, int T, int F, int* out_len, hipStream_t s);

// ---- attention (attention.hip: lane-split kernels, routes, launchers; attention_mfma.hip / attention_bwd_mfma.hip: the MFMA kernels) ----
// q,k [B,H,T,dh], vt [B,H,dh,T]; o [B*T, H*dh]; lse [B,H,T]
// maskbits: attn_mask_words(B, H, T) dwords where the MFMA forward kernel stores the dropout keep flags for the backward
// kernels (nullptr: the backward kernels hash again; the lane-split kernels always hash)
size_t attn_mask_words(int B, int H, int T);
// bias [T, T] f32 (row = query, added to the scaled score, finite or -inf) and key_len [B] int32 (keys >= key_len[b] masked; clamped to
// [0, T] in the kernel): device arrays, either may be nullptr; one of them given = a masked call (attention_masked.hip), both nullptr = today's kernels
int launch_attn_fwd(int dt, const void* q, const void* k, const void* vt, void* o, float* lse,
                    int B, int H, int T, int dh, float scale, DropSpec drop, int impl, uint32_t* maskbits, hipStream_t s,
                    const float* bias = nullptr, const int* key_len = nullptr);
// dqkv [B*T, 3*H*dh] packed like the qkv projection output (head_major flag as in EpiArgs)
int launch_attn_bwd(int dt, const void* q, const void* k, const void* vt, const void* o, const void* dout,
                    const float* lse, float* delta, void* dqkv, int B, int H, int T, int dh, float scale,
                    DropSpec drop, int head_major, int impl, uint32_t* maskbits, hipStream_t s,
                    const float* bias = nullptr, const int* key_len = nullptr);
// The kernel a call runs on (attention.hip: the one place that decides and that reads g_attn_bwd_two_pass / ISHARA_NO_ATTN_BITS); the
// launchers and the name functions are switches over it.  impl: 0 lane-split, 1 MFMA where there is one; drop: dropout is active
// (DropSpec.thr != 0); bits: the caller gave a keep-bit buffer; head_major: the dqkv packing; masked: a bias table or key lengths are given
// ATT_LANE: attn_fwd_kernel, or the attn_bwd_dq / _dkv pair; ATT_LANE_MASKED: the same three with the masks (attention_masked.hip);
// ATT_MFMA_MASKED / ATT_BWD_TWO_KERNEL_MASKED: the masked mode of the MFMA forward / of the MFMA kernel pair (the one-pass backward has none)
enum AttnKind { ATT_REFUSED, ATT_LANE, ATT_MFMA, ATT_MFMA_F16, ATT_BWD_TWO_KERNEL, ATT_BWD_FUSED, ATT_LANE_MASKED, ATT_MFMA_MASKED, ATT_BWD_TWO_KERNEL_MASKED };
// why: the refusal's message; dm: the MFMA kernels' dropout mode 0 / 1 / 2; nw, nt, full: waves, key tiles per wave and T == 16 nw nt of ATT_BWD_FUSED
// bias16: a masked kernel that reads the bias table with 16-byte loads (the table must be 16-byte aligned)
struct AttnRoute { AttnKind kind; const char* why; int dm, nw, nt; bool full, bias16; };
AttnRoute attn_fwd_route(int dt, int T, int dh, int impl, bool drop, bool bits, bool masked = false);
AttnRoute attn_bwd_route(int dt, int T, int dh, int impl, bool drop, bool bits, bool head_major, bool masked = false);
// the kernel's rocprof name with its template arguments ("" when refused; a kernel pair as "dq + dkv<...>"); valid until the next call
const char* attn_fwd_kernel_name(int dt, int T, int dh, int impl, bool drop, bool bits, bool masked = false);
const char* attn_bwd_kernel_name(int dt, int T, int dh, int impl, bool drop, bool bits, bool head_major, bool masked = false);
// what the masked kernels share: the key count of clip b (key_len clamped to [0, T]; T without key lengths), and the lse they store for a
// FULLY MASKED row (l = 0 at the end: o = 0): large and finite, so that the backward kernels recompute P = exp(s - lse) = 0 for every key
#define ATT_DEAD_LSE 1e30f
DEVI int attn_key_count(const int* __restrict__ key_len, int b, int Tn) { return key_len ? min(max(key_len[b], 0), Tn) : Tn; }
template <int N> struct att_int { static constexpr int v = N; };      // a template argument chosen at run time: fn(att_int<N>{})
// the lane-split launches (attention.hip, attention_masked.hip): fn(E{}, att_int<DHL>{}) in the storage type (F16: fp16 too, the unmasked forward only)
// and at DHL = dh / 4, which the route has passed
template <bool F16, typename F> static int att_lane(int dt, int dh, F fn) {
    auto at = [&](auto e) {
        dh == 8 ? fn(e, att_int<2>{}) : dh == 16 ? fn(e, att_int<4>{}) : dh == 24 ? fn(e, att_int<6>{}) : dh == 32 ? fn(e, att_int<8>{}) : dh == 48 ? fn(e, att_int<12>{}) : fn(e, att_int<16>{});
        return launch_rc();
    };
    if constexpr (F16) if (dt == DT_F16) return at(f16{});
    return dt == DT_BF16 ? at(bf16{}) : at(float{});
}
// the MFMA kernels behind ATT_MFMA / ATT_MFMA_F16 (attention_mfma.hip) and ATT_BWD_TWO_KERNEL / ATT_BWD_FUSED (attention_bwd_mfma.hip)
int launch_attn_fwd_mfma(int dm, const void* q, const void* k, const void* vt, void* o, float* lse,
                         int B, int H, int T, int dh, float scale, DropSpec drop, uint32_t* maskbits, hipStream_t s);
int launch_attn_fwd_mfma_f16(const void* q, const void* k, const void* vt, void* o, float* lse, int B, int H, int T, int dh, float scale, hipStream_t s);
int launch_attn_bwd_mfma(const AttnRoute& r, const void* q, const void* k, const void* vt, const void* o, const void* dout, const float* lse,
                         float* delta, void* dqkv, int B, int H, int T, int dh, float scale, DropSpec drop, uint32_t* maskbits, hipStream_t s);
// the masked modes behind ATT_MFMA_MASKED (attention_mfma.hip) and ATT_BWD_TWO_KERNEL_MASKED (attention_bwd_mfma.hip): dm 0 / 1
int launch_attn_fwd_mfma_masked(int dm, const void* q, const void* k, const void* vt, void* o, float* lse, const float* bias, const int* key_len,
                                int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s);
int launch_attn_bwd_mfma_masked(int dm, const void* q, const void* k, const void* vt, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                                const float* bias, const int* key_len, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s);
// the masked lane-split kernels behind ATT_LANE_MASKED (attention_masked.hip): f32 / bf16, the lane-split head dims, any T
int launch_attn_fwd_lane_masked(int dt, const void* q, const void* k, const void* vt, void* o, float* lse, const float* bias, const int* key_len,
                                int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s);
int launch_attn_bwd_lane_masked(int dt, const void* q, const void* k, const void* vt, const void* o, const void* dout, const float* lse, float* delta,
                                void* dqkv, const float* bias, const int* key_len, int B, int H, int T, int dh, float scale, DropSpec drop, int head_major,
                                hipStream_t s);

// ---- CTC / decode (ctc.hip) ----------------------------------------------------------
size_t ctc_workspace_floats(int B, int T, int L);
// the dynamic LDS one workgroup of the loss kernel asks for (lse[T] + the extended labels) and the most a launch grants it
size_t ctc_lds_bytes(int T, int L);
size_t ctc_lds_limit();
// logits [B,T,C] f32; labels [B,L] int64 (padded with blank); nll [B]; dlogits = grad_scale * d nll_b / d logits
int launch_ctc(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank,
               float* nll, float* dlogits, float grad_scale, float* ws, hipStream_t s, void* dlb = nullptr);
// per-sample frame counts (device frame_len [B] int32 or NULL: T each; outside [1, T]: a sample without frames), a per-sample factor on
// grad_scale (sample_scale [B] f32 or NULL) and zero_inf: an infeasible sample's gradient is +0.  T stays the stride (contract: ishara_hip.h)
int launch_ctc_len(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, float* nll, float* dlogits,
                   float grad_scale, float* ws, const int* frame_len, const float* sample_scale, int zero_inf, hipStream_t s);
// ---- gradient of the n-best scores (ctc_nbest_grad.hip) and the MWER weights (mwer_weights.hip): contracts in ishara_hip.h.  The launchers
// check nothing: ctc_nbest_grad_check holds the refusals of ishara_ctc_nbest_grad (0: go ahead; B == 0 passes and launches nothing)
int64_t ctc_nbest_grad_workspace_bytes(int B, int T, int N, int max_len);
int ctc_nbest_grad_check(const char* fn, const float* logits, int B, int T, int C, int blank, const int* hyp_idx, const int* hyp_len, int N, int Th,
                         int max_len, const int* frame_len, const float* coef, const float* dlogits, const void* dlb, const float* logp,
                         const int* status, const void* ws);
int launch_ctc_nbest_grad(const float* logits, int B, int T, int C, int blank, const int* hyp_idx, const int* hyp_len, int N, int Th, int max_len,
                          const int* frame_len, const float* coef, float grad_scale, float* dlogits, int accumulate, void* dlb, float* logp,
                          int* status, void* ws, hipStream_t s);
int launch_mwer_weights(const int* hyp_idx, const int* hyp_len, const float* logp, const int* status, int B, int N, int Th, const int* targets, int L,
                        const float* inv_temp, int mode, int* dist, float* post, float* risk, float* coef, int* tlen, hipStream_t s);
// ---- gradient of the distillation term (kd_grad.hip): contract in ishara_hip.h.  The launcher checks nothing: kd_grad_check holds the
// refusals of ishara_kd_grad (0: go ahead; B == 0 passes and launches nothing)
int kd_grad_check(const char* fn, const float* logits, const float* teacher, int B, int T, int C, float inv_temp, int mode, const int* frame_len,
                  float grad_scale, const float* dlogits, int accumulate, const void* dlb, const float* kl_frame, const float* kl_clip);
int launch_kd_grad(const float* logits, const float* teacher, int B, int T, int C, float inv_temp, int mode, const int* frame_len, float grad_scale,
                   float* dlogits, int accumulate, void* dlb, float* kl_frame, float* kl_clip, hipStream_t s);
int launch_fill_u32(void* p, size_t n_words, uint32_t v, hipStream_t s);   // model.hip
int launch_mean(const float* v, float* out, int n, float scale, hipStream_t s);
int launch_greedy_decode(const float* logits, int B, int T, int C, int blank, int* out_idx, int* out_len, hipStream_t s);
int launch_greedy_decode_len(const float* logits, int B, int T, int C, int blank, int* out_idx, int* out_len, const int* frame_len, hipStream_t s);

// ---- inference preprocessing (preprocess.hip): raw [max_frames,276] (+ device clip length) -> [T,276]; mean/std [276] in OUTPUT order
int launch_preprocess(const float* raw, const int* n_frames, int max_frames, const float* mean, const float* stdv, float* out, int T, hipStream_t s);
// batched ragged form: raw [N_total,276] packed clips, offsets [B+1] int64 (device) -> out [B,T,276]; both buffers 16-byte aligned
int launch_preprocess_batch(const float* raw, int64_t n_total, const int64_t* offsets, int B, int max_frames, const float* mean, const float* stdv,
                            float* out, int T, hipStream_t s);
// ---- test-set scoring (score.hip): edit distance of greedy decodes (len < 3 -> fallback phrase) to pad-59 targets [B,L], L <= 64
#define SCORE_MAX_L 64
int launch_edit_distance(const int* out_idx, const int* out_len, int B, int T, const int* targets, int L, int* dist, int* tlen, hipStream_t s);
// ---- edit-operation alignment (score_align.hip): the canonical edit script of the same pairs -> ops [B,4], aligned [B,L], inserted [B,L+1] and
// confusion [60,60] (+=, may be null); fallback != 0 applies the len < 3 rule; ws = edit_alignment_workspace_bytes(B, T), 16-byte aligned
size_t edit_alignment_workspace_bytes(int B, int T);
int launch_edit_alignment(const int* out_idx, const int* out_len, int B, int T, const int* targets, int L, int fallback, int* ops, int* aligned,
                          int* inserted, int* confusion, void* ws, hipStream_t s);
// ---- CTC prefix beam search (ctc_beam.hip): logits [B,T,C] f32 -> n-best prefixes; ws = B * ctc_beam_workspace_words(T, W) int32 (trie)
__host__ __device__ size_t ctc_beam_workspace_words(int T, int W);
int launch_ctc_beam(const float* logits, int B, int T, int C, int blank, int W, int nbest, const float* lm, float alpha, float beta,
                    void* ws, int* out_idx, int* out_len, float* out_score, hipStream_t s);
int launch_ctc_beam_len(const float* logits, int B, int T, int C, int blank, int W, int nbest, const float* lm, float alpha, float beta,
                        void* ws, int* out_idx, int* out_len, float* out_score, const int* frame_len, hipStream_t s);
// the LM as an automaton: lm_logp f32 / lm_next i32 [S,C] on the device, one state per beam; frame_len may be null
int launch_ctc_beam_lm(const float* logits, int B, int T, int C, int blank, int W, int nbest, const float* lm_logp, const int* lm_next, int S,
                       int start_state, float alpha, float beta, void* ws, int* out_idx, int* out_len, float* out_score, const int* frame_len,
                       hipStream_t s);
// ---- CTC forced alignment (ctc_align.hip): the best path of a known label, per-symbol frame spans and confidences (ishara_amd/ctc_align.py)
bool ctc_align_bp_in_lds(int T, int L);                          // the back-pointers (T * 128 bytes) fit in LDS: the workspace is not used
size_t ctc_align_workspace_bytes(int B, int T, int L);
int launch_ctc_align(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, void* ws, int* frame_pos, int* start,
                     int* end, float* conf, float* score, hipStream_t s);
int launch_ctc_align_len(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, void* ws, int* frame_pos, int* start,
                         int* end, float* conf, float* score, const int* frame_len, hipStream_t s);
// ---- training input batch (input_batch.hip): device store of raw clips + per-clip augmentation table -> x [B,T,F]
#define CLIP_MAX_T 4096
int launch_clip_batch(const float* raw, const ishara_clip_aug* clips, int B, int T, int layout, float* x, hipStream_t s);
// the same with the spatial affine, the temporal mask and the per-clip frame count (input_batch_ex.hip); frame_len may be null
int launch_clip_batch_ex(const float* raw, const ishara_clip_aug_ex* clips, int B, int T, int layout, float* x, int* frame_len, hipStream_t s);

// ---- optimizer (optimizer.hip) -----------------------------------------------------------
struct RAdamArgs { float lr, wd, beta1, beta2, eps, c1, c2, r_t; int rect; int sync; float slow_step; };
int launch_radam_lookahead(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n,
                           RAdamArgs a, hipStream_t s);
// the same update reading the device record of launch_grad_stats: g = grad[i] * st->coef; skip != 0 and st->nonfinite > 0: nothing is
// written but st->skipped += 1
int launch_radam_lookahead_ex(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n,
                              RAdamArgs a, ishara_grad_stats* st, int skip, hipStream_t s);
int launch_scale(float* x, int64_t n, float scale, hipStream_t s);
// the host-side scalars of step `iteration` (1-based): bias corrections, rectification, the Lookahead sync flag
RAdamArgs radam_args(int32_t iteration, float lr, float wd);
// Parameter groups: the same update over the segment table of awp.hip (seg_off device int64 [S + 1]) with one device row per segment:
// a frozen segment is neither read nor written, another steps with lr * lr_scale and wd * wd_scale.  theta, grad, m, v, slow at 16-byte
// aligned addresses; st may be null (then skip must be 0); ws of param_groups_workspace_bytes(n, S) bytes, 8-byte aligned, written by
// every call before it is read.  Two launches each: the chunk table, then the pass.  grad_mask_groups: g = +0.0f over the frozen segments.
int64_t param_groups_workspace_bytes(int64_t n, int32_t S);
int launch_radam_lookahead_groups(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, RAdamArgs a, ishara_grad_stats* st,
                                  int skip, const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, hipStream_t s);
int launch_grad_mask_groups(float* g, int64_t n, const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, hipStream_t s);

// ---- gradient statistics and accumulation (grad_ops.hip) ------------------------------------
// g, acc [n] f32 at 16-byte aligned addresses, 1 <= n <= 2^31 - 1; ws: grad_stats_workspace_bytes(n) bytes, 8-byte aligned, needs no
// initialisation (every row read was written by the same call)
int64_t grad_stats_workspace_bytes(int64_t n);
int launch_grad_stats(const float* g, int64_t n, float grad_scale, float clip_norm, ishara_grad_stats* out, void* ws, hipStream_t s);
int launch_grad_accumulate(float* acc, const float* g, int64_t n, int first, hipStream_t s);

// ---- exponential moving average of the weights (weight_avg.hip) -----------------------------
// avg, theta, a, b [n] f32 at 16-byte aligned addresses, disjoint, 1 <= n <= 2^31 - 1; rec 8-byte aligned, zeroed once by its owner.
// weight_average: two launches, the update and, behind it, one thread that writes the record (see the file for why); st may be null
// when skip == 0.  weight_swap exchanges the two buffers as 32-bit words.
int launch_weight_average(float* avg, float* theta, int64_t n, float momentum, int warmup, int overwrite_every, ishara_ema_state* rec,
                          const ishara_grad_stats* st, int skip, hipStream_t s);
int launch_weight_swap(float* a, float* b, int64_t n, hipStream_t s);

// ---- adversarial weight perturbation (awp.hip) ------------------------------------------------
// w, backup [n] f32 at 16-byte aligned addresses, disjoint; g [n] f32 (16-byte accesses when its address allows them); seg_off device int64
// [S + 1], 0 = seg_off[0] < ... < seg_off[S] = n (the caller's contract: the host cannot read it); scale device [S]; ws of
// awp_workspace_bytes(n, S) bytes at an 8-byte aligned address.  awp_norms: four launches (chunk table, chunk sums, per-segment scale,
// the record); awp_apply behind it on the same stream with the same ws / seg_off / S / n: backup = w, w += scale[s] * g.
int64_t awp_workspace_bytes(int64_t n, int32_t S);
int launch_awp_norms(const float* w, const float* g, const int64_t* seg_off, int32_t S, int64_t n, float delta, float eps, int relative, float* scale,
                     ishara_awp_stats* rec, void* ws, hipStream_t s);
int launch_awp_apply(float* w, float* backup, const float* g, const int64_t* seg_off, int32_t S, int64_t n, const float* scale, void* ws, hipStream_t s);
int launch_awp_restore(float* w, const float* backup, int64_t n, hipStream_t s);
