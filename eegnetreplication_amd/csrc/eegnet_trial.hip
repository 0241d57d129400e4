// eegnet_trial.hip -- the per-trial building blocks of the whole-trial kernels: k_infer (eval forward,
// eegnet_passes.hip), k_eval_folds (fold-indexed validation, eegnet_eval_folds.hip), k_infer_dx (eval-mode
// input gradients, eegnet_input_grad.hip) and k_frozen (frozen-BatchNorm fine-tuning, eegnet_frozen.hip).
// Included by eegnet_kernels.hip (one translation unit).
//
// The four run a whole EEGNet trial on one CU in one layout: 1024 threads = 16 waves, one workgroup per
// trial in flight, trials strided over the grid.  Wave o owns row o of every per-trial [F2, T] plane
// (F2 <= 16), so its FIR taps are wave-uniform (SGPRs) and the FIR windows it reads are lane-contiguous
// float4s; a lane of it holds pooled samples t = lane + 64 m (m < MAXT1Q) of the block-2 rows.  The next
// trial's x is fetched into registers at the top of a trial and stored over the x rows after their last
// reader.  The pads of every padded row are zeroed once and never written, so nothing of a trial (a NaN
// included) reaches the next one.  No piece below has a kernel-specific branch; what a kernel adds (a
// stored plane, a dropout factor, gradient sums) is its own code or a callback.
//
// k_infer and k_eval_folds share the operand load and the whole trial (infer_ops_load, infer_trial, at the
// end of this file).  k_infer_dx and k_frozen are built from the pieces in between.  infer_trial does not
// call those pieces: it spells the same steps out, because every one of them -- trial_lds included -- moved
// the register allocation of some k_infer / k_eval_folds instantiation when infer_trial went through it,
// and the eval forward is the kernel whose time is benchmarked (profiles/trial_body_refactor.txt).

namespace eeg {

// ---- LDS plan (float offsets into the dynamic LDS) ----
//     Xs  [C][RS]     x rows
//     Ss  [F2][RS]    s rows
//     Ps  [F2][RS]    PLANE only: a second full-rate plane (k_infer_dx: ELU'(z2); k_frozen: v)
//     D2s [F2][RS2]   d2 rows, left pad LP2
//     Qs  [F2][RS2]   q rows
//     Hs  [NF up to 4]
//     Lg  [NCLS]      the trial's logits, for the kernels that read them back
// [0, Hs) are the padded rows a kernel zeroes at entry.  make_geo sizes the launches from the same
// function: ldsI = the plain plan up to Lg (k_infer; k_eval_folds adds NCLS), ldsX = the PLANE plan
// with Lg (k_infer_dx, k_frozen).
struct TrialLds {
    int Ss, Ps, D2s, Qs, Hs, Lg, n;
};
__host__ __device__ constexpr TrialLds trial_lds(int C, int F2, int RS, int RS2, int NF, bool plane) {
    TrialLds L{};
    L.Ss = C * RS;
    L.Ps = L.Ss + F2 * RS;
    L.D2s = L.Ps + (plane ? F2 * RS : 0);
    L.Qs = L.D2s + F2 * RS2;
    L.Hs = L.Qs + F2 * RS2;
    L.Lg = L.Hs + ((NF + 3) & ~3);
    L.n = L.Lg + NCLS;
    return L;
}

// ---- per-model operands ----
// what a workgroup keeps in registers of one model: the spatial MFMA fragment, and of wave o's row the
// temporal taps, block-2 weights and the folded BatchNorm maps z2 = al v + be, z3 = s3 r + b3
template <int K1, int KS_>
struct InferOps {
    float aw[KS_];
    float tap[K1];
    float w2[K2], w3[F2MAX];
    float al, be, s3, b3;
};

// a wave-uniform parameter load: plain (kernel-argument pointers: the compiler proves it scalar), or
// SC = true through the constant address space (ldc) for pointers that come from a fold record and
// loads that follow the kernel's own stores, which would otherwise land in one VGPR per value
template <bool SC>
__device__ __forceinline__ float ld_w(const float* p) {
    if constexpr (SC) return ldc(p);
    else return *p;
}

// the weights of InferOps alone, for k_frozen, which folds its BatchNorm maps itself (see infer_ops_load)
template <int K1, int CC, int TT, int FF, bool SC, int KS_>
__device__ __forceinline__ void infer_weights_load(const Geo& g, const float* __restrict__ prm, int wave, int lane,
                                                   InferOps<K1, KS_>& w) {
    EEG_DIMS(g);
    static_assert(KS_ == KS, "InferOps: k-steps of the spatial fragment");
    load_ws_frag<KS>(prm + g.o_ws, C, F2, w.aw, lane);
    const int oo = wave < F2 ? wave : 0, gg = oo / g.D;
#pragma unroll
    for (int k = 0; k < K1; ++k) w.tap[k] = ld_w<SC>(prm + (g.o_w1 + gg * K1 + k));
#pragma unroll
    for (int k = 0; k < K2; ++k) w.w2[k] = ld_w<SC>(prm + (g.o_w2 + oo * K2 + k));
#pragma unroll
    for (int i = 0; i < F2MAX; ++i) w.w3[i] = i < F2 ? ld_w<SC>(prm + (g.o_W3 + oo * F2 + i)) : 0.f;
}

// the eval kernels' operands: the weights and the eval BatchNorm fold.  The scales are g / sqrtf(rv + eps);
// k_frozen, whose backward needs 1 / sd on its own, rounds g * (1 / sqrtf(..)) and keeps its own fold
template <int K1, int CC, int TT, int FF, bool SC, int KS_>
__device__ __forceinline__ void infer_ops_load(const Geo& g, const float* __restrict__ prm,
                                               const float* __restrict__ bn, int wave, int lane,
                                               InferOps<K1, KS_>& w) {
    EEG_DIMS(g);
    static_assert(KS_ == KS, "InferOps: k-steps of the spatial fragment");
    const float* rm1 = bn;                 const float* rv1 = bn + g.F1;
    const float* rm2 = bn + 2 * g.F1;      const float* rv2 = rm2 + F2;
    const float* rm3 = rm2 + 2 * F2;       const float* rv3 = rm3 + F2;
    load_ws_frag<KS>(prm + g.o_ws, C, F2, w.aw, lane);
    const int o = wave;
    const int oo = o < F2 ? o : 0, gg = oo / g.D;
#pragma unroll
    for (int k = 0; k < K1; ++k) w.tap[k] = ld_w<SC>(prm + (g.o_w1 + gg * K1 + k));
#pragma unroll
    for (int k = 0; k < K2; ++k) w.w2[k] = ld_w<SC>(prm + (g.o_w2 + oo * K2 + k));
#pragma unroll
    for (int i = 0; i < F2MAX; ++i) w.w3[i] = i < F2 ? ld_w<SC>(prm + (g.o_W3 + oo * F2 + i)) : 0.f;
    // eval BN1 (model.py:32) and BN2 (model.py:47) folded: z2 = al * v + be; BN3: z3 = s3 r + b3
    {
        const float a1 = ld_w<SC>(prm + (g.o_g1 + gg)) / sqrtf(ld_w<SC>(rv1 + gg) + g.eps);
        const float c1 = ld_w<SC>(prm + (g.o_b1 + gg)) - a1 * ld_w<SC>(rm1 + gg);
        float W = 0.f;
        for (int c = 0; c < C; ++c) W += ld_w<SC>(prm + (g.o_ws + oo * C + c));
        const float s2 = ld_w<SC>(prm + (g.o_g2 + oo)) / sqrtf(ld_w<SC>(rv2 + oo) + g.eps);
        w.al = a1 * s2;
        w.be = (c1 * W - ld_w<SC>(rm2 + oo)) * s2 + ld_w<SC>(prm + (g.o_b2 + oo));
        w.s3 = ld_w<SC>(prm + (g.o_g3 + oo)) / sqrtf(ld_w<SC>(rv3 + oo) + g.eps);
        w.b3 = ld_w<SC>(prm + (g.o_b3 + oo)) - ld_w<SC>(rm3 + oo) * w.s3;
    }
}

// ---- trial loop ----
// A kernel's first trial x0 into the x rows (`on`, wave-uniform: the workgroup has a trial at all).  The
// first barrier orders the store behind the kernel's zeroing of the pads (and a previous model's readers).
// In the loop a kernel calls x_prefetch for the next trial at the top and x_store behind the last reader of
// its x rows.
template <int PF_>
__device__ __forceinline__ void trial_x_first(bool on, const float* __restrict__ x0, int C, int T, int RS, int LP,
                                              float* Xs, float (&pf)[PF_], int tid) {
    if (on) x_prefetch<PF_>(x0, C, T, pf, tid);
    __syncthreads();
    x_store<PF_>(pf, C, T, RS, LP, Xs, tid);
    __syncthreads();
    drain_prologue_loads();
}

// ---- forward pieces ----
// wave o's s row -> v = FIR_w1(s), four samples at a time; quad(q, v) returns d2[q] (and stores what else
// the kernel keeps of the quad)
template <int K1, typename Quad>
__device__ __forceinline__ void temporal_row(const float* srow, float* drow, int T1, const float (&tap)[K1],
                                             int lane, Quad&& quad) {
    using G_ = KG<K1>;
    for (int q = lane; q < T1; q += 64) {
        float win[4 * G_::NW];
        lds_window<G_::NW>(srow + 4 * q, win);
        float v[4];
        fir4<K1, G_::OFF>(win, tap, v);
        drow[q] = quad(q, v);
    }
}
// pool4(ELU(al v + be)) of one quad
__device__ __forceinline__ float elu_pool4(float al, float be, const float (&v)[4]) {
    float pe = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) pe += elu_f(fmaf(al, v[i], be));
    return pe * 0.25f;
}

// block_2 of one trial: the padded d2 rows (D2s) -> depthwise q[t] = sum_k w2[k] d2[t + k - 7] into the q
// rows -> pointwise r = W3 q.  Qq is sample 0 of q row 0 (the rows of k_infer_dx and k_frozen carry a
// left pad for what lands on them later).  Returns r[m] for t = lane + 64 m of row o.  Contains one
// workgroup barrier.
__device__ __forceinline__ void block2_rows(int F2, int T1, int RS2, const float* D2s, float* Qq,
                                            const float (&w2)[K2], const float (&w3)[F2MAX], bool row_on,
                                            int o, int lane, float (&r)[MAXT1Q]) {
    if (row_on) {
        const float* dr = D2s + o * RS2 + 1;
#pragma unroll
        for (int m = 0; m < MAXT1Q; ++m) {
            const int t = lane + 64 * m;
            if (t < T1) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < K2; ++k) a = fmaf(w2[k], dr[t + k], a);
                Qq[o * RS2 + t] = a;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < MAXT1Q; ++m) {
        const int t = lane + 64 * m;
        float a = 0.f;
        if (row_on && t < T1) {
#pragma unroll
            for (int i = 0; i < F2MAX; ++i)
                if (i < F2) a = fmaf(w3[i], Qq[i * RS2 + t], a);
        }
        r[m] = a;
    }
}

// h = pool8(ELU(s3 r + b3)) keep(j) into Hs; keep(j) is the dropout factor of pooled sample j of row o (1 in
// eval mode).  The 8-lane sums are three DPP steps (xor 1, xor 2, half-row mirror).
template <typename Keep>
__device__ __forceinline__ void pool8_head(int T2, float* Hs, float s3, float b3, const float (&r)[MAXT1Q],
                                           bool row_on, int o, int lane, Keep&& keep) {
#pragma unroll
    for (int m = 0; m < MAXT1Q; ++m) {
        const int t = lane + 64 * m;
        const bool on = row_on && t < 8 * T2;
        float e = on ? elu_f(fmaf(s3, r[m], b3)) : 0.f;
        e += dpp<0xB1>(e);
        e += dpp<0x4E>(e);
        e += dpp<0x141>(e);
        if (on && (t & 7) == 0) Hs[o * T2 + (t >> 3)] = e * 0.125f * keep(t >> 3);
    }
}

// logits = Wfc h + bfc: wave n < NCLS computes logit n, its lane 0 calls out(n, logit)
template <typename Out>
__device__ __forceinline__ void classifier(const Geo& g, const float* __restrict__ prm, const float* Hs, int NF,
                                           int wave, int lane, Out&& out) {
    if (wave < NCLS) {
        const int n = wave;
        float a = 0.f;
        for (int i = lane; i < NF; i += 64) a = fmaf(prm[g.o_Wfc + n * NF + i], Hs[i], a);
        a = wave_sum(a);
        if (lane == 0) out(n, a + prm[g.o_bfc + n]);
    }
}

// the max, exponentials and their sum of a trial's four logits: softmax = ex / sum, logsumexp = mx + logf(sum)
__device__ __forceinline__ float softmax4(const float (&l)[NCLS], float (&ex)[NCLS], float& mx) {
    mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
    float sum = 0.f;
#pragma unroll
    for (int n = 0; n < NCLS; ++n) { ex[n] = expf(l[n] - mx); sum += ex[n]; }
    return sum;
}

// ---- backward pieces ----
// a lane's MAXT1Q samples of wave o's block-2 row, registers -> LDS (row: sample 0)
__device__ __forceinline__ void row_store(float* row, int T1, int lane, const float (&v)[MAXT1Q]) {
#pragma unroll
    for (int m = 0; m < MAXT1Q; ++m) {
        const int t = lane + 64 * m;
        if (t < T1) row[t] = v[m];
    }
}

// dq[o,t] = sum_i W3[i,o] dr[i,t] in registers; Dr is sample 0 of dr row 0, w3c = &W3[0][o]
__device__ __forceinline__ void w3t_rows(const float* __restrict__ w3c, int F2, int T1, int RS2, const float* Dr,
                                         int lane, float (&dq)[MAXT1Q]) {
#pragma unroll
    for (int m = 0; m < MAXT1Q; ++m) {
        const int t = lane + 64 * m;
        float a = 0.f;
        if (t < T1) {
#pragma unroll
            for (int i = 0; i < F2MAX; ++i)
                if (i < F2) a = fmaf(w3c[i * F2], Dr[i * RS2 + t], a);
        }
        dq[m] = a;
    }
}

// transposed depthwise FIR dd2[q] = sum_k w2[k] dq[q - k + 7]; qb is sample 7 of the dq row (pads swapped: 8 | 7)
__device__ __forceinline__ float fir16_t(const float (&w2)[K2], const float* qb, int q) {
    float a = 0.f;
#pragma unroll
    for (int k = 0; k < K2; ++k) a = fmaf(w2[k], qb[q - k], a);
    return a;
}

// transposed temporal FIR ds[t] = sum_k w1[k] d[t - k + P] of wave o's row: the forward FIR with the taps
// flipped, pads R | P.  `row` is the padded operand row, dsrow sample 0 of the result row, tapl tap `lane`.
// One or two quads past a multiple of 64 (22 x 257: quad 64 holds the one sample t = 256) would cost a
// whole window pass with one or two lanes on: the lane-parallel loop stops at NQF and those samples are
// 64-lane dot products instead, lane k on tap k.
template <int K1>
__device__ __forceinline__ void temporal_row_t(const float* row, float* dsrow, int T, int TQ,
                                               const float (&tap)[K1], float tapl, int lane) {
    using G_ = KG<K1>;
    constexpr int LP = G_::LP;
    const int NQF = (TQ >= 64 && (TQ & 63) != 0 && (TQ & 63) <= 2) ? (TQ & ~63) : TQ;
    for (int q = lane; q < NQF; q += 64) {
        float w[4 * G_::NW];
        lds_window<G_::NW>(row + 4 * q, w);
        floatx4 d;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < K1; ++k) a = fmaf(tap[K1 - 1 - k], w[G_::OFFD + i + k], a);
            d[i] = 4 * q + i < T ? a : 0.f;
        }
        lds_st4(dsrow + 4 * q, d);
    }
    if (NQF < TQ) {
        for (int t = 4 * NQF; t < 4 * TQ; ++t) {
            float p = (lane < K1 && t < T) ? tapl * row[LP + t + G_::P - lane] : 0.f;
            p = wave_sum(p);
            if (lane == 0) dsrow[t] = p;
        }
    }
}

// ---- the eval forward of one trial ----
// The trial's x rows are in the workgroup's x buffer: its four logits go to out(n, logit), called by lane 0
// of wave n.  xn (wave-uniform, NULL: none) is the next trial: its x is fetched into pf at the top and
// stored over the x rows once their last reader, the spatial GEMM, is done.  Ends in a barrier.
template <int K1, int CC, int TT, int FF, int KS_, int PF_, typename Out>
__device__ __forceinline__ void infer_trial(const Geo& g, const float* __restrict__ prm,
                                            const InferOps<K1, KS_>& w, float* sm,
                                            const float* __restrict__ xn, float (&pf)[PF_], int tid, int wave,
                                            int lane, Out&& out) {
    EEG_DIMS(g);
    static_assert(KS_ == KS && PF_ == PF, "infer_trial: fragment / prefetch sizes of this shape");
    float* Ss = sm + C * RS;
    float* D2s = Ss + F2 * RS;
    float* Qs = D2s + F2 * RS2;
    float* Hs = Qs + F2 * RS2;
    const int o = wave;
    const bool row_on = o < F2;
    if (xn) x_prefetch<PF>(xn, C, T, pf, tid);
    spatial_mfma<KS>(sm, w.aw, Ss, C, F2, NT16, RS, LP, wave, lane);
    __syncthreads();
    if (row_on) {
        using G_ = KG<K1>;
        const float* row = Ss + o * RS;
        float* drow = D2s + o * RS2 + LP2;
        for (int q = lane; q < T1; q += 64) {
            float win[4 * G_::NW];
            lds_window<G_::NW>(row + 4 * q, win);
            float v[4];
            fir4<K1, G_::OFF>(win, w.tap, v);
            float pe = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) pe += elu_f(fmaf(w.al, v[i], w.be));
            drow[q] = pe * 0.25f;
        }
    }
    if (xn) x_store<PF>(pf, C, T, RS, LP, sm, tid);
    __syncthreads();
    float r[MAXT1Q];
    block2_rows(F2, T1, RS2, D2s, Qs, w.w2, w.w3, row_on, o, lane, r);
#pragma unroll
    for (int m = 0; m < MAXT1Q; ++m) {
        const int t = lane + 64 * m;
        float e = (row_on && t < 8 * T2) ? elu_f(fmaf(w.s3, r[m], w.b3)) : 0.f;
        e += dpp<0xB1>(e);                 // 8-lane sums by DPP (xor 1, xor 2, half-row mirror)
        e += dpp<0x4E>(e);
        e += dpp<0x141>(e);
        if (row_on && (t & 7) == 0 && t < 8 * T2) Hs[o * T2 + (t >> 3)] = e * 0.125f;
    }
    __syncthreads();
    if (wave < NCLS) {
        const int n = wave;
        float a = 0.f;
        for (int i = lane; i < NF; i += 64) a = fmaf(prm[g.o_Wfc + n * NF + i], Hs[i], a);
        a = wave_sum(a);
        if (lane == 0) out(n, a + prm[g.o_bfc + n]);
    }
    __syncthreads();
}

}  // namespace eeg
