// eegnet_frozen.hip -- frozen-BatchNorm fine-tuning: the fused forward + loss + backward + parameter
// gradient kernel behind eegnet_frozen_step / eegnet_forward_frozen, and the reduction of its
// per-workgroup partial rows; their fold-indexed instantiations (FOLD: blockIdx.y is the model) and the
// fold-indexed Adam behind eegnet_frozen_step_folds; and the instantiations that read their batch as windows of
// continuous recordings in place (FzWin, behind eegnet_frozen_step_windows: eegnet_windows.hip's table loader).
// Included by eegnet_kernels.hip (one translation unit).
//
// With the BatchNorm layers frozen (running statistics used and left untouched, dropout still on)
// every trial is independent: none of the five batch-global reductions that split the train step into
// passes A..E exist, and the whole chain of a trial stays on one CU.  With
// a1 = g1/sd1, c1 = b1 - a1 rm1, W_o = sum_c ws[o,c], s2 = g2/sd2, s3 = g3/sd3:
//     forward   s = ws x;  v = FIR_w1(s);  u = a1 v + c1 W_o;  z2 = s2 (u - rm2) + b2
//               d2 = pool4(ELU(z2)) m2/(1-p);  q = FIR_w2(d2);  r = W3 q
//               z3 = s3 (r - rm3) + b3;  h = pool8(ELU(z3)) m3/(1-p);  logits = Wfc h + bfc
//     seed      g = dlogits[b]  or  (softmax(logits[b]) - onehot(label[b])) / B   (loss += CE/B)
//     backward  dWfc += g (x) h;  dbfc += g;  dh = Wfc^T g;  dz3 = dh/8 m3/(1-p) ELU'(z3)
//               dg3 += sum dz3 (r - rm3)/sd3;  db3 += sum dz3;  dr = s3 dz3
//               dW3 += dr q^T;  dq = W3^T dr;  dw2[o,k] += sum_t dq[o,t] d2[o,t+k-7];  dd2 = FIR^T_w2(dq)
//               dz2 = dd2/4 m2/(1-p) ELU'(z2);  dg2 += sum dz2 (u - rm2)/sd2;  db2 += sum dz2;  du = s2 dz2
//               dg1[g] += sum_{o in g} sum_t du (v - rm1 W_o)/sd1;  db1[g] += sum_{o in g} W_o sum_t du
//               dw1[g,k] += a1 sum_{o in g} sum_t du[o,t] s[o,t+k-P]
//               dws[o,c] += a1 sum_t ds'[o,t] x[c,t] + c1 sum_t du[o,t],   ds' = FIR^T_w1(du)
// k_frozen is a whole-trial kernel: the layout, the weight operands and the forward and transposed pieces
// are eegnet_trial.hip's, in its PLANE LDS plan (make_geo's ldsX); the BatchNorm fold is its own (the
// backward needs 1/sd2 and 1/sd3 on their own, and s2 = g2 (1/sd2) rounds differently from g2/sd2).  Its rows:
//     Xs   x rows, kept until the dws product
//     Ss   s rows; after the dw1 correlation, ds'
//     Ps   v rows; then du
//     D2s  d2 rows
//     Qs   q rows; then dr (all rows are read by every wave), then dq
//
// Gradient sums.  Everything a lane can keep cheaply stays in registers across the workgroup's trials
// (the per-row BatchNorm sums, the classifier products, the dws MFMA accumulators); the three lag /
// channel correlations (dw1, dw2, dW3) are reduced over the wave once per trial and added, by a fixed
// lane in trial order, to the workgroup's own partial row in global memory.  The partial row holds raw
// sums (FzCols); k_frozen_reduce sums the rows over the workgroups in workgroup order in fp64, applies
// the trial-invariant factors (a1, c1, W_o, 1/sd1), sums the rows of a temporal group, clamps and writes
// `grads` and `loss`.  No atomics anywhere: the bits depend on the launch grid, not on scheduling.

namespace eeg {

// columns of one workgroup's partial row (floats)
struct FzCols {
    int w1;     // [F2][K1]  sum_t du[o,t] s[o,t+k-P]
    int dv;     // [F2]      sum_t du v
    int su;     // [F2]      sum_t du
    int ws;     // [F2][C]   sum_t ds'[o,t] x[c,t]
    int g2, b2; // [F2]
    int w2;     // [F2][16]
    int W3;     // [F2][F2]
    int g3, b3; // [F2]
    int Wfc;    // [4][NF]
    int bfc;    // [4]
    int loss;   // [1]
    int n;
};
__host__ __device__ inline FzCols fz_cols(const Geo& g) {
    FzCols c;
    int o = 0;
    c.w1 = o; o += g.F2 * g.K1;
    c.dv = o; o += g.F2;
    c.su = o; o += g.F2;
    c.ws = o; o += g.F2 * g.C;
    c.g2 = o; o += g.F2;
    c.b2 = o; o += g.F2;
    c.w2 = o; o += g.F2 * K2;
    c.W3 = o; o += g.F2 * g.F2;
    c.g3 = o; o += g.F2;
    c.b3 = o; o += g.F2;
    c.Wfc = o; o += NCLS * g.NF;
    c.bfc = o; o += NCLS;
    c.loss = o; o += 1;
    c.n = o;
    return c;
}

// this workgroup's running sum in its partial row: a plain store for its first trial (the row needs no
// zeroing), a read-modify-write by the same lane afterwards
__device__ __forceinline__ void fz_add(float* p, float v, bool first) { *p = first ? v : *p + v; }

// db2 += dz2 = a e of a cut stage, rounded as the stage-0 instantiation of the same shape rounds its
// `aB2 += dz2`: the compiler contracts that statement into fma(a, e, aB2) in the run-time-shape
// instantiations and keeps the rounded product and a plain add in the compile-time-shape ones (SPEC), where
// the sum is scheduled behind the du store.  Stage 0 must stay the code it was, so the cut stages spell
// out either form; tests/test_gpu_partial_finetune.py compares the bits with stage 0 for both kinds.
template <bool SPEC>
__device__ __forceinline__ float fz_b2_add(float acc, float a, float e) {
    if constexpr (SPEC) {
#pragma clang fp contract(off)
        const float dz2 = a * e;
        return acc + dz2;
    } else {
        return fmaf(a, e, acc);
    }
}

// The last argument of the frozen kernels: nothing for a single model; the call of a fold-indexed launch
// (eegnet_frozen_step_folds), where blockIdx.y is the fold and its parameters, BN buffers, x, labels,
// permutation and partial rows come from folds[blockIdx.y] (the pointer arguments are then unused).
template <bool FOLD> struct FzFold {};
template <> struct FzFold<true> { FoldCall fc; };

// The loader policy of k_frozen, its last template parameter and the type of its last argument.  FzFold<FOLD>
// (the default) takes batch row b from x as a contiguous [C][T] trial: xrow / x_prefetch / trial_x_first.
// FzWin (eegnet_frozen_step_windows) takes it from a table of windows of continuous recordings, read where
// they lie: batch row b is table entry e = sel ? clamp(sel[b], 0, ac.total - 1) : b, its x the window
// win_org(ac, C, T, e) places (start and recording clamped into the recordings, load width per window) and
// its label lab[e]; dlogits, logits, the injected masks and the dropout counters stay indexed by b.
// win_prefetch fills the registers x_prefetch would fill from the window copied out, so everything behind
// the loader carries the bits of the default policy on the copy.
struct FzWin {
    WinAtCall ac;                 // total: the table's length
    const long long* sel;         // [B] table entries of the batch, device, nullable (entry b)
};
template <class Src> constexpr bool fz_is_win = false;
template <> constexpr bool fz_is_win<FzWin> = true;

// table entry of batch row b (wave-uniform)
__device__ __forceinline__ int fz_entry(const FzWin& fw, int b) {
    if (!fw.sel) return b;
    long long e = fw.sel[b];
    e = e < 0 ? 0 : e >= fw.ac.total ? fw.ac.total - 1 : e;
    return (int)e;
}

// the windowed loader's x_prefetch: batch row b's window, at its clamped origin and load width.  (A function
// that takes C, T and tid by value, not a by-reference lambda in the kernel: with the lambda every
// compile-time-shape kernel that calls x_store -- the pre-existing ones included -- came out 8 to 36 bytes
// longer, its x_store index arithmetic no longer folded)
template <int PF>
__device__ __forceinline__ void fz_win_prefetch(const FzWin& fw, int C, int T, int b, float (&pf)[PF], int tid) {
    const WinOrg org = win_org(fw.ac, C, T, fz_entry(fw, b));
    win_prefetch<PF>(org.row0, fw.ac.pitch, org.vec, C, T, pf, tid);
}

// STAGE (EEGNET_TRAIN_*): the first trainable module in network order.  The flat parameter buffer is in
// network order, so the trainable set is the suffix [o_g2 | o_w2 | o_Wfc, nparam) of it, and the backward of
// a trial stops as soon as the last sum of that suffix is complete:
//     1 (aggregation)  ... dq -> dd2 -> dz2 for dg2 / db2 alone: no du, no dv / su sums, no dw1 correlation,
//                      no ds', no dws product (and none of their registers: aWs, c1w, tapl)
//     2 (block_2)      ... dW3, dq (registers) and dw2: no dd2, no dz2; dq is never stored
//     3 (classifier)   the seed, dbfc, dWfc and the loss: no dz3, no LDS row reused
// A cut instantiation writes only the partial-row columns of its suffix (FzCols unchanged: one workspace
// serves every stage), and k_frozen_reduce reads only those.  What is computed is computed by the same
// statements in the same order as in stage 0, so the suffix sums have the same bits.
// Workgroup barriers of the backward, per stage (the forward's four are every stage's):
//     q rows read: dr may land        stages 0-2   Qs is reused: every wave reads all q rows for dW3
//     dr rows complete                stages 0-2   w3t_rows reads every wave's dr row
//     dr rows read: dq may land       stages 0-1   stage 2 keeps dq in registers and leaves the dr rows alone
//     ds' rows complete               stage 0      the dws product reads every ds' row
//     x rows read (end of trial)      stage 0      the dws product is the last reader of Xs; in the cut
//                                                  stages that is spatial_mfma, four barriers earlier
//     next x stored (end of trial)    every stage  spatial_mfma of the next trial reads all x rows; it is
//                                                  also what keeps Hs / Lg / Qs / D2s of this trial from the
//                                                  next one's writers
constexpr int FZ_ALL = 0, FZ_AGG = 1, FZ_B2 = 2, FZ_CLS = 3;
template <int K1, int CC, int TT, int FF, bool BWD, bool FOLD = false, int STAGE = FZ_ALL, class Src = FzFold<FOLD>>
__global__ __launch_bounds__(NTH) void k_frozen(Geo g, const float* __restrict__ prm,
                                                const float* __restrict__ bn, const float* __restrict__ x,
                                                const float* __restrict__ dlog, const int64_t* __restrict__ lab,
                                                const uint8_t* __restrict__ m2, const uint8_t* __restrict__ m3,
                                                float* __restrict__ logits, float* part, Src fold) {
    using G_ = KG<K1>;
    constexpr bool WIN = fz_is_win<Src>;                // x and the labels through a table of windows (x unused)
    static_assert(!(WIN && FOLD), "the windowed loader serves the single-model step");
    EEG_DIMS(g);
    // fold launch: the batch is rows perm[row0 ...] (or row0 ...) of the fold's x / labels, seeded by the
    // mean cross-entropy, its dropout key mix(seed, koff + *step) as a KEY_FROM_STEP single call's
    // (row0 is folded into the pointers -- perm, or x and labels without one -- so one pointer stays live)
    const int64_t* perm = nullptr;
    unsigned key0 = 0u, key1 = 0u;
    if constexpr (FOLD) {
        const eegnet_fold f = fold_rec(fold.fc);
        prm = f.params; bn = f.bn_buffers; part = (float*)f.ws;
        dlog = nullptr; m2 = nullptr; m3 = nullptr; logits = nullptr;
        perm = f.perm ? f.perm + fold.fc.row0 : nullptr;
        x = f.perm ? f.x : f.x + (size_t)fold.fc.row0 * ((size_t)C * T);
        lab = f.perm ? f.labels : f.labels + fold.fc.row0;
        if (g.drop) { key0 = fold_drop_key(fold.fc, f, 0); key1 = fold_drop_key(fold.fc, f, 1); }
    }
    constexpr int NCTM = CC ? (CC + 15) / 16 : 4;      // 16-channel tiles of the dws product (C <= 64)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const TrialLds L = trial_lds(C, F2, RS, RS2, NF, true);
    float* const Xs = sm;
    float* const Ss = sm + L.Ss;
    float* const Vs = sm + L.Ps;
    float* const D2s = sm + L.D2s;
    float* const Qs = sm + L.Qs;
    float* const Hs = sm + L.Hs;
    float* const Lg = sm + L.Lg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const float* rm1 = bn;                 const float* rv1 = bn + g.F1;
    const float* rm2 = bn + 2 * g.F1;      const float* rv2 = rm2 + F2;
    const float* rm3 = rm2 + 2 * F2;       const float* rv3 = rm3 + F2;

    for (int i = tid; i < L.Hs; i += NTH) sm[i] = 0.f;
    InferOps<K1, KS> w;
    infer_weights_load<K1, CC, TT, FF, false>(g, prm, wave, lane, w);
    const int o = wave;
    const bool row_on = o < F2;
    const int oo = row_on ? o : 0, gg = oo / g.D;
    const float tapl = lane < K1 ? prm[g.o_w1 + gg * K1 + lane] : 0.f;     // tap `lane` (the ds' tail samples)
    // frozen BN1 and BN2 folded: z2 = al v + be, (u - rm2)/sd2 = ax v + bx; BN3: z3 = s3 r + b3
    float ax, bx, s2, i3, m3o;
    {
        const float a1 = prm[g.o_g1 + gg] / sqrtf(rv1[gg] + g.eps);
        const float c1 = prm[g.o_b1 + gg] - a1 * rm1[gg];
        float W = 0.f;
        for (int c = 0; c < C; ++c) W += prm[g.o_ws + oo * C + c];
        const float i2 = 1.f / sqrtf(rv2[oo] + g.eps);
        s2 = prm[g.o_g2 + oo] * i2;
        w.al = a1 * s2;
        w.be = (c1 * W - rm2[oo]) * s2 + prm[g.o_b2 + oo];
        ax = a1 * i2;
        bx = (c1 * W - rm2[oo]) * i2;
        i3 = 1.f / sqrtf(rv3[oo] + g.eps);
        w.s3 = prm[g.o_g3 + oo] * i3;
        m3o = rm3[oo];
        w.b3 = prm[g.o_b3 + oo] - m3o * w.s3;
    }
    const float al = w.al, be = w.be, s3 = w.s3, b3 = w.b3;
    if constexpr (!FOLD) { key0 = g.drop ? drop_key(g, 0) : 0u; key1 = g.drop ? drop_key(g, 1) : 0u; }
    const float invB = 1.f / (float)g.B;
    // sums kept in registers across this workgroup's trials
    float aG3 = 0.f, aB3 = 0.f, aG2 = 0.f, aB2 = 0.f, aDV = 0.f, aSU = 0.f, aLoss = 0.f;
    float aFc[NCLS] = {0.f, 0.f, 0.f, 0.f}, aBfc[NCLS] = {0.f, 0.f, 0.f, 0.f};
    floatx4 aWs[STAGE == FZ_ALL ? NCTM : 1];            // (never touched by a cut stage)
    if constexpr (STAGE == FZ_ALL) {
#pragma unroll
        for (int ct = 0; ct < NCTM; ++ct) aWs[ct] = (floatx4){0.f, 0.f, 0.f, 0.f};
    }
    const FzCols fc = fz_cols(g);
    float* const prow = BWD ? part + (size_t)blockIdx.x * fc.n : nullptr;

    const size_t nx = (size_t)C * T;
    // trial b of the batch in x (and, with the same row index, in labels)
    auto xrow = [&](auto b) {
        if constexpr (FOLD) return x + (size_t)fold_row(perm, 0, (int)b) * nx;
        else return x + (size_t)b * nx;
    };
    float pf[PF];
    // (xrow is evaluated before the guard, a perm[] load included: the host launches min(B, CUs) workgroups,
    // so blockIdx.x < g.B in every launch and the guard only mirrors the other kernels')
    if constexpr (WIN) {                                   // trial_x_first on the first window
        if ((int)blockIdx.x < g.B) fz_win_prefetch<PF>(fold, C, T, blockIdx.x, pf, tid);
        __syncthreads();
        x_store<PF>(pf, C, T, RS, LP, Xs, tid);
        __syncthreads();
        drain_prologue_loads();
    } else {
        trial_x_first<PF>((int)blockIdx.x < g.B, xrow(blockIdx.x), C, T, RS, LP, Xs, pf, tid);
    }

    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        const int bnx = b + gridDim.x;
        const bool first = b == (int)blockIdx.x;
        if constexpr (WIN) {
            if (bnx < g.B) fz_win_prefetch<PF>(fold, C, T, bnx, pf, tid);
        } else {
            if (bnx < g.B) x_prefetch<PF>(xrow(bnx), C, T, pf, tid);
        }
        // ---------------- forward ----------------
        spatial_mfma<KS>(Xs, w.aw, Ss, C, F2, NT16, RS, LP, wave, lane);
        __syncthreads();                                   // s rows complete
        const unsigned i2b = ((unsigned)b * (unsigned)F2 + (unsigned)oo) * (unsigned)T1;
        const unsigned i3b = ((unsigned)b * (unsigned)F2 + (unsigned)oo) * (unsigned)T2;
        if (row_on) {
            float* vrow = Vs + o * RS + LP;
            temporal_row<K1>(Ss + o * RS, D2s + o * RS2 + LP2, T1, w.tap, lane, [&](int q, const float (&v)[4]) {
                lds_st4(vrow + 4 * q, (floatx4){v[0], v[1], v[2], v[3]});
                return elu_pool4(al, be, v) * keep_mul(g, m2, key0, i2b + (unsigned)q);
            });
            wave_lds_fence();
        }
        float r[MAXT1Q];
        block2_rows(F2, T1, RS2, D2s, Qs + LP2, w.w2, w.w3, row_on, o, lane, r);
        pool8_head(T2, Hs, s3, b3, r, row_on, o, lane,
                   [&](int j) { return keep_mul(g, m3, key1, i3b + (unsigned)j); });
        __syncthreads();                                   // h complete
        classifier(g, prm, Hs, NF, wave, lane, [&](int n, float l) {
            Lg[n] = l;
            if (logits) logits[(size_t)b * NCLS + n] = l;
        });
        __syncthreads();                                   // logits of this trial in Lg
        if constexpr (BWD) {
            // ---------------- seed g = dL/dlogits of this trial ----------------
            float gs[NCLS];
            if (dlog) {
#pragma unroll
                for (int n = 0; n < NCLS; ++n) gs[n] = dlog[(size_t)b * NCLS + n];
            } else {                                       // mean cross-entropy: (softmax - onehot) / B
                float l[NCLS];
#pragma unroll
                for (int n = 0; n < NCLS; ++n) l[n] = Lg[n];
                int cls;
                if constexpr (WIN) cls = (int)lab[fz_entry(fold, b)];      // the label follows the table entry
                else cls = (int)lab[FOLD ? fold_row(perm, 0, b) : (long long)b];
                float ex[NCLS], mx, lc = 0.f;
                const float sum = softmax4(l, ex, mx);
#pragma unroll
                for (int n = 0; n < NCLS; ++n) {
                    gs[n] = (ex[n] / sum - (n == cls ? 1.f : 0.f)) * invB;
                    lc = n == cls ? l[n] : lc;
                }
                aLoss += (logf(sum) + mx - lc) * invB;
            }
            // ---------------- backward ----------------
#pragma unroll
            for (int n = 0; n < NCLS; ++n) aBfc[n] += gs[n];
            if (tid < NF) {
                const float h = Hs[tid];
#pragma unroll
                for (int n = 0; n < NCLS; ++n) aFc[n] = fmaf(gs[n], h, aFc[n]);
            }
            if constexpr (STAGE < FZ_CLS) {
                float drv[MAXT1Q];
                if (row_on) {
                    // dz3 = dh/8 m3/(1-p) ELU'(z3), dh = Wfc^T g; BN3 sums; dr = s3 dz3 (registers)
                    const float* wfc = prm + g.o_Wfc + o * T2;
#pragma unroll
                    for (int m = 0; m < MAXT1Q; ++m) {
                        const int t = lane + 64 * m;
                        float v = 0.f;
                        if (t < 8 * T2) {
                            float dh = 0.f;
#pragma unroll
                            for (int n = 0; n < NCLS; ++n) dh = fmaf(wfc[n * NF + (t >> 3)], gs[n], dh);
                            const float dz3 = 0.125f * dh * keep_mul(g, m3, key1, i3b + (unsigned)(t >> 3)) *
                                              elu_d(fmaf(s3, r[m], b3));
                            aG3 = fmaf(dz3, (r[m] - m3o) * i3, aG3);
                            aB3 += dz3;
                            v = s3 * dz3;
                        }
                        drv[m] = v;
                    }
                    // dW3[o,i] += sum_t dr[o,t] q[i,t]
                    float cw[F2MAX];
#pragma unroll
                    for (int i = 0; i < F2MAX; ++i) cw[i] = 0.f;
#pragma unroll
                    for (int m = 0; m < MAXT1Q; ++m) {
                        const int t = lane + 64 * m;
                        if (t < 8 * T2) {
#pragma unroll
                            for (int i = 0; i < F2MAX; ++i)
                                if (i < F2) cw[i] = fmaf(drv[m], Qs[i * RS2 + LP2 + t], cw[i]);
                        }
                    }
                    wave_reduce<F2MAX>(cw);                    // lane 16 r: sum[j + 4 r] in cw[j]
                    if (li == 0) {
#pragma unroll
                        for (int j = 0; j < F2MAX / 4; ++j) {
                            const int i = j + (F2MAX / 4) * lk;
                            if (i < F2) fz_add(prow + fc.W3 + o * F2 + i, cw[j], first);
                        }
                    }
                }
                __syncthreads();                               // the q rows are read: dr may land on them
                if (row_on) row_store(Qs + o * RS2 + LP2, T1, lane, drv);
                __syncthreads();                               // dr rows complete
                float dqv[MAXT1Q];
                if (row_on) w3t_rows(prm + g.o_W3 + o, F2, T1, RS2, Qs + LP2, lane, dqv);
                if constexpr (STAGE < FZ_B2) __syncthreads();  // dr rows read: dq may land on them
                if (row_on) {
                    if constexpr (STAGE < FZ_B2) row_store(Qs + o * RS2 + LP2, T1, lane, dqv);
                    // dw2[o,k] += sum_t dq[o,t] d2[o,t+k-7]
                    const float* dr = D2s + o * RS2 + 1;
                    float cw[K2];
#pragma unroll
                    for (int k = 0; k < K2; ++k) cw[k] = 0.f;
#pragma unroll
                    for (int m = 0; m < MAXT1Q; ++m) {
                        const int t = lane + 64 * m;
                        if (t < T1) {
#pragma unroll
                            for (int k = 0; k < K2; ++k) cw[k] = fmaf(dqv[m], dr[t + k], cw[k]);
                        }
                    }
                    wave_reduce<K2>(cw);
                    if (li == 0) {
#pragma unroll
                        for (int j = 0; j < K2 / 4; ++j)
                            fz_add(prow + fc.w2 + o * K2 + j + (K2 / 4) * lk, cw[j], first);
                    }
                    if constexpr (STAGE < FZ_B2) {
                        wave_lds_fence();
                        // dz2[4q + i] = dd2[q]/4 m2/(1-p) ELU'(z2[4q + i]); BN2 / BN1 sums; du = s2 dz2 over the v row
                        const float* qb = Qs + o * RS2 + (LP2 + 7);
                        float* vrow = Vs + o * RS + LP;
                        for (int q = lane; q < T1; q += 64) {
                            float a = fir16_t(w.w2, qb, q);
                            a *= 0.25f * keep_mul(g, m2, key0, i2b + (unsigned)q);
                            const floatx4 v = lds_ld4(vrow + 4 * q);
                            floatx4 du;
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                const float e = elu_d(fmaf(al, v[i], be));
                                const float dz2 = a * e;
                                aG2 = fmaf(dz2, fmaf(ax, v[i], bx), aG2);
                                if constexpr (STAGE == FZ_ALL) aB2 += dz2;
                                else aB2 = fz_b2_add<TT != 0>(aB2, a, e);
                                if constexpr (STAGE == FZ_ALL) {
                                    const float d = s2 * dz2;
                                    aDV = fmaf(d, v[i], aDV);
                                    aSU += d;
                                    du[i] = d;
                                }
                            }
                            if constexpr (STAGE == FZ_ALL) lds_st4(vrow + 4 * q, du);
                        }
                        if constexpr (STAGE == FZ_ALL) {
                            // (samples [4 T1, T) of the v row are never written: du is zero there, as it has to be)
                            wave_lds_fence();
                            // dw1 raw correlation: sum_t du[o,t] s[o,t+k-P], 32 lags at a time
                            const float* srow = Ss + o * RS;
                            constexpr int NWC = (G_::OFF + 32 + 6) / 4;
#pragma unroll
                            for (int kc = 0; kc < K1; kc += 32) {
                                float c1w[32];
#pragma unroll
                                for (int k = 0; k < 32; ++k) c1w[k] = 0.f;
                                for (int q = lane; q < T1; q += 64) {
                                    float win[4 * NWC];
                                    lds_window<NWC>(srow + 4 * q + kc, win);
                                    const floatx4 du = lds_ld4(vrow + 4 * q);
#pragma unroll
                                    for (int k = 0; k < 32; ++k)
#pragma unroll
                                        for (int i = 0; i < 4; ++i) c1w[k] = fmaf(du[i], win[G_::OFF + i + k], c1w[k]);
                                }
                                wave_reduce<32>(c1w);                  // lane 16 r: sum[j + 8 r] in c1w[j]
                                if (li == 0) {
#pragma unroll
                                    for (int j = 0; j < 8; ++j)
                                        fz_add(prow + fc.w1 + o * K1 + kc + j + 8 * lk, c1w[j], first);
                                }
                            }
                            wave_lds_fence();
                            // ds' = FIR^T_w1(du) over the s row (its last reader was the correlation above)
                            temporal_row_t<K1>(Vs + o * RS, Ss + o * RS + LP, T, TQ, w.tap, tapl, lane);
                        }
                    }
                }
            }
            if constexpr (STAGE == FZ_ALL) {
                __syncthreads();                               // ds' rows complete
                // dws raw product sum_t ds'[o,t] x[c,t]: v_mfma_f32_16x16x4_f32, A = ds' tile (16 o x 4 t),
                // B = x tile (4 t x 16 c), D[o = 4 (l >> 4) + r][c = 16 ct + (l & 15)]; wave w takes the
                // 4-sample steps w, w + 16, ... and keeps its accumulators across the trials
                for (int ks = wave; ks < TQ; ks += NWAVE) {
                    const int t = 4 * ks + lk;
                    const float av = li < F2 ? Ss[li * RS + LP + t] : 0.f;
#pragma unroll
                    for (int ct = 0; ct < NCTM; ++ct) {
                        if (ct < NCT) {
                            const int c = 16 * ct + li;
                            const float bv = c < C ? Xs[c * RS + LP + t] : 0.f;
                            aWs[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, aWs[ct], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // x rows read: the next trial's x may land (a cut stage's last reader of them is spatial_mfma)
        if constexpr (!BWD || STAGE == FZ_ALL) __syncthreads();
        if (bnx < g.B) x_store<PF>(pf, C, T, RS, LP, Xs, tid);
        __syncthreads();
    }

    if constexpr (BWD) {
        // ---------------- publish this workgroup's partial row ----------------
        if constexpr (STAGE == FZ_ALL) {
            aG3 = wave_sum(aG3); aB3 = wave_sum(aB3); aG2 = wave_sum(aG2); aB2 = wave_sum(aB2);
            aDV = wave_sum(aDV); aSU = wave_sum(aSU);
            if (row_on && lane == 0) {
                prow[fc.g3 + o] = aG3; prow[fc.b3 + o] = aB3; prow[fc.g2 + o] = aG2; prow[fc.b2 + o] = aB2;
                prow[fc.dv + o] = aDV; prow[fc.su + o] = aSU;
            }
        } else if constexpr (STAGE < FZ_CLS) {             // the columns of the trainable suffix alone
            aG3 = wave_sum(aG3); aB3 = wave_sum(aB3);
            if constexpr (STAGE == FZ_AGG) { aG2 = wave_sum(aG2); aB2 = wave_sum(aB2); }
            if (row_on && lane == 0) {
                prow[fc.g3 + o] = aG3; prow[fc.b3 + o] = aB3;
                if constexpr (STAGE == FZ_AGG) { prow[fc.g2 + o] = aG2; prow[fc.b2 + o] = aB2; }
            }
        }
        if (tid < NF) {
#pragma unroll
            for (int n = 0; n < NCLS; ++n) prow[fc.Wfc + n * NF + tid] = aFc[n];
        }
        if (tid == 0) {
#pragma unroll
            for (int n = 0; n < NCLS; ++n) prow[fc.bfc + n] = aBfc[n];
            prow[fc.loss] = aLoss;
        }
        // the waves' dws accumulators summed in wave order through the (free) x rows
        if constexpr (STAGE == FZ_ALL) {
        for (int w = 0; w < NWAVE; ++w) {
            if (wave == w) {
#pragma unroll
                for (int ct = 0; ct < NCTM; ++ct) {
                    if (ct < NCT) {
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr) {
                            const int oa = 4 * lk + rr, c = 16 * ct + li;
                            if (oa < F2 && c < C) {
                                const int i = oa * C + c;
                                sm[i] = (w == 0 ? 0.f : sm[i]) + aWs[ct][rr];
                            }
                        }
                    }
                }
            }
            __syncthreads();
        }
        for (int i = tid; i < F2 * C; i += NTH) prow[fc.ws + i] = sm[i];
        }   // STAGE == FZ_ALL
    }
}

// Sum of the partial rows over the workgroups, in workgroup order and fp64, turned into `grads` (flat
// parameter layout) and `loss`.  One output element per lane; the four waves of a workgroup take a
// quarter of the rows each and their sums are added in row order, so the result is a function of the
// partial rows alone.  `off` is the first element of the trainable suffix (0: every parameter): the grid
// covers [off, nparam] -- the suffix and the loss --, element e is computed as in the full launch whatever
// `off`, and neither grads[0 : off) nor a partial-row column of a frozen parameter is touched (a cut
// k_frozen leaves those columns unwritten).
// FOLD: blockIdx.y is the fold, whose rows, parameters, BN buffers, `grads` and loss slot come from its record.
constexpr int NTFR = 256, FR_OUT = 64;
template <bool FOLD = false>
__global__ __launch_bounds__(NTFR) void k_frozen_reduce(Geo g, const float* __restrict__ prm,
                                                        const float* __restrict__ bn,
                                                        const float* __restrict__ part, int nrows,
                                                        float* __restrict__ grads, float* __restrict__ loss,
                                                        int off, FzFold<FOLD> fold) {
    if constexpr (FOLD) {
        const eegnet_fold f = fold_rec(fold.fc);
        prm = f.params; bn = f.bn_buffers; part = (const float*)f.ws; grads = f.grads;
        loss = f.losses ? f.losses + fold.fc.slot : nullptr;
    }
    __shared__ double sh[NTFR / FR_OUT][FR_OUT];
    const FzCols fc = fz_cols(g);
    const int tid = threadIdx.x, le = tid & (FR_OUT - 1), qd = tid / FR_OUT;
    const int e = off + blockIdx.x * FR_OUT + le;
    const int w0 = (int)((long long)qd * nrows / (NTFR / FR_OUT)), w1 = (int)((long long)(qd + 1) * nrows / (NTFR / FR_OUT));
    auto col = [&](int c) {
        double s = 0.0;
        const float* p = part + c;
#pragma unroll 8
        for (int w = w0; w < w1; ++w) s += (double)p[(size_t)w * fc.n];
        return s;
    };
    auto Wsum = [&](int o) {
        double W = 0.0;
        for (int c = 0; c < g.C; ++c) W += (double)prm[g.o_ws + o * g.C + c];
        return W;
    };
    auto inv1 = [&](int gq) { return 1.0 / sqrt((double)bn[g.F1 + gq] + (double)g.eps); };
    double acc = 0.0;
    if (e <= g.nparam) {
        if (e < g.o_g1) {                                  // temporal.0.weight [F1][K1]
            const int gq = e / g.K1, k = e - gq * g.K1;
            for (int d = 0; d < g.D; ++d) acc += col(fc.w1 + (gq * g.D + d) * g.K1 + k);
            acc *= (double)prm[g.o_g1 + gq] * inv1(gq);
        } else if (e < g.o_b1) {                           // temporal.1.weight [F1]
            const int gq = e - g.o_g1;
            for (int d = 0; d < g.D; ++d) {
                const int o = gq * g.D + d;
                acc += col(fc.dv + o) - (double)bn[gq] * Wsum(o) * col(fc.su + o);
            }
            acc *= inv1(gq);
        } else if (e < g.o_ws) {                           // temporal.1.bias [F1]
            const int gq = e - g.o_b1;
            for (int d = 0; d < g.D; ++d) {
                const int o = gq * g.D + d;
                acc += Wsum(o) * col(fc.su + o);
            }
        } else if (e < g.o_g2) {                           // spatial.weight [F2][C]
            const int i = e - g.o_ws, o = i / g.C, gq = o / g.D;
            const double a1 = (double)prm[g.o_g1 + gq] * inv1(gq);
            const double c1 = (double)prm[g.o_b1 + gq] - a1 * (double)bn[gq];
            acc = a1 * col(fc.ws + i) + c1 * col(fc.su + o);
        } else if (e < g.o_b2) acc = col(fc.g2 + (e - g.o_g2));
        else if (e < g.o_w2) acc = col(fc.b2 + (e - g.o_b2));
        else if (e < g.o_W3) acc = col(fc.w2 + (e - g.o_w2));
        else if (e < g.o_g3) acc = col(fc.W3 + (e - g.o_W3));
        else if (e < g.o_b3) acc = col(fc.g3 + (e - g.o_g3));
        else if (e < g.o_Wfc) acc = col(fc.b3 + (e - g.o_b3));
        else if (e < g.o_bfc) acc = col(fc.Wfc + (e - g.o_Wfc));
        else if (e < g.nparam) acc = col(fc.bfc + (e - g.o_bfc));
        else acc = col(fc.loss);
    }
    sh[qd][le] = acc;
    __syncthreads();
    if (qd == 0 && e <= g.nparam) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < NTFR / FR_OUT; ++j) s += sh[j][le];
        float v = (float)s;
        if (e == g.nparam) {
            if (loss) *loss = v;
        } else {
            if (!g.noclamp) {
                if (e >= g.o_ws && e < g.o_g2) v = fminf(fmaxf(v, -1.0f), 1.0f);             // model.py:44
                else if (e >= g.o_Wfc && e < g.o_bfc) v = fminf(fmaxf(v, -0.25f), 0.25f);    // model.py:84
            }
            grads[e] = v;
        }
    }
}

// k_adam for every fold of a fold-indexed frozen step (blockIdx.y the fold): the same element update with
// the same scalars, so a fold's parameters and Adam state come out as eegnet_adam_step leaves them.  A
// fold without Adam state keeps its parameters.  The step counters are advanced by k_step_inc_folds, a
// launch of its own behind this one: every workgroup here reads its fold's counter.  Elements [off, n) are
// updated (off: the first trainable element); parameters and both moments below `off` are not touched.
__global__ __launch_bounds__(256) void k_adam_folds(int64_t n, int64_t off, FoldCall fc) {
    const eegnet_fold f = fold_rec(fc);
    if (!f.adam_state) return;
    const int s = *f.step + 1;
    const int64_t i = off + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const float step_size = (float)((double)fc.lr / (1.0 - pow((double)fc.b1, (double)s)));
        const float bc2s = (float)sqrt(1.0 - pow((double)fc.b2, (double)s));
        adam_elem(f.params + i, f.grads[i], f.adam_state + i, f.adam_state + n + i, fc.b1, fc.b2, step_size, bc2s,
                  fc.eps);
    }
}

__global__ __launch_bounds__(256) void k_step_inc_folds(FoldCall fc, int nfolds) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < nfolds && fc.folds[k].adam_state) *fc.folds[k].step += 1;
}

}  // namespace eeg
