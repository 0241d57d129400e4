// eegnet_input_grad.hip -- eval-mode input gradients (saliency): the fused forward + dL/dx kernel
// behind eegnet_input_grad_eval.  Included by eegnet_kernels.hip (one translation unit).
//
// In eval mode BatchNorm is affine with the running statistics and there is no dropout, so every trial
// is independent and dx is the transposed chain of what k_infer computes:
//     forward   s = ws x;  v = FIR_w1(s);  z2 = al v + be;  d2 = pool4(ELU(z2));  q = FIR_w2(d2);
//               r = W3 q;  z3 = s3 r + b3;  h = pool8(ELU(z3));  logits = Wfc h + bfc
//     backward  dh = Wfc^T g;  dr = s3 dh/8 ELU'(z3);  dq = W3^T dr;  dd2 = FIR^T_w2(dq);
//               dz2 = dd2/4 ELU'(z2);  ds = FIR^T_w1(al dz2);  dx = ws^T ds
// k_infer_dx is a whole-trial kernel: the layout, the operands and the forward and transposed pieces are
// eegnet_trial.hip's, in its PLANE LDS plan (make_geo's ldsX).  A trial never leaves the CU between x
// and dx, and its rows are reused as it goes:
//     Xs   x rows; after the spatial GEMM has read them, the staging rows of dx
//     Ss   s rows; then al dz2 (the operand of the transposed temporal FIR)
//     Ps   al/4 ELU'(z2); then ds (the B operand of the dx GEMM)
//     D2s  d2 rows; then dr
//     Qs   q rows; then dq
// ELU'(z3) is recomputed from r, which a lane still holds in registers when the seed arrives.

namespace eeg {

template <int K1, int CC, int TT, int FF>
__global__ __launch_bounds__(NTH) void k_infer_dx(Geo g, const float* __restrict__ prm,
                                                  const float* __restrict__ bn, const float* __restrict__ x,
                                                  int kind, const float* __restrict__ dlog,
                                                  const int64_t* __restrict__ tgt, float* __restrict__ dx,
                                                  float* __restrict__ logits, int vec) {
    EEG_DIMS(g);
    constexpr int NCTM = CC ? (CC + 15) / 16 : 4;      // 16-channel tiles of the dx GEMM (C <= 64)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const TrialLds L = trial_lds(C, F2, RS, RS2, NF, true);
    float* const Xs = sm;
    float* const Ss = sm + L.Ss;
    float* const Es = sm + L.Ps;
    float* const D2s = sm + L.D2s;
    float* const Qs = sm + L.Qs;
    float* const Hs = sm + L.Hs;
    float* const Lg = sm + L.Lg;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;

    for (int i = tid; i < L.Hs; i += NTH) sm[i] = 0.f;
    InferOps<K1, KS> w;
    infer_ops_load<K1, CC, TT, FF, false>(g, prm, bn, wave, lane, w);
    // the transposed spatial fragment of the dx GEMM: A[c = 16 ct + (l & 15)][o = 4 s + (l >> 4)]
    float awT[NCTM][4];
#pragma unroll
    for (int ct = 0; ct < NCTM; ++ct)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int c = 16 * ct + li, oa = 4 * s + lk;
            awT[ct][s] = (c < C && oa < F2) ? prm[g.o_ws + oa * C + c] : 0.f;
        }
    const int o = wave;
    const bool row_on = o < F2;
    const int oo = row_on ? o : 0, gg = oo / g.D;
    const float tapl = lane < K1 ? prm[g.o_w1 + gg * K1 + lane] : 0.f;     // tap `lane` (the ds tail samples)
    const float al4 = 0.25f * w.al;
    const size_t nx = (size_t)C * T;
    float pf[PF];
    trial_x_first<PF>((int)blockIdx.x < g.B, x + (size_t)blockIdx.x * nx, C, T, RS, LP, Xs, pf, tid);

    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        const int bnx = b + gridDim.x;
        if (bnx < g.B) x_prefetch<PF>(x + (size_t)bnx * nx, C, T, pf, tid);
        // ---------------- forward ----------------
        spatial_mfma<KS>(Xs, w.aw, Ss, C, F2, NT16, RS, LP, wave, lane);
        __syncthreads();                                   // s rows complete; the x rows are free
        if (row_on) {
            float* erow = Es + o * RS + LP;
            temporal_row<K1>(Ss + o * RS, D2s + o * RS2 + LP2, T1, w.tap, lane, [&](int q, const float (&v)[4]) {
                float pe = 0.f;
                floatx4 e;
#pragma unroll
                for (int i = 0; i < 4; ++i) {              // ELU and ELU' share the exponential
                    const float z = fmaf(w.al, v[i], w.be), ez = fast_exp(z);
                    pe += z > 0.f ? z : ez - 1.f;
                    e[i] = z > 0.f ? al4 : al4 * ez;       // al/4 ELU'(z2)
                }
                lds_st4(erow + 4 * q, e);
                return pe * 0.25f;
            });
            wave_lds_fence();
        }
        float r[MAXT1Q];
        block2_rows(F2, T1, RS2, D2s, Qs + LP2, w.w2, w.w3, row_on, o, lane, r);
        pool8_head(T2, Hs, w.s3, w.b3, r, row_on, o, lane, [](int) { return 1.f; });
        __syncthreads();                                   // h complete
        classifier(g, prm, Hs, NF, wave, lane, [&](int n, float l) {
            Lg[n] = l;
            if (logits) logits[(size_t)b * NCLS + n] = l;
        });
        __syncthreads();                                   // logits of this trial in Lg
        // ---------------- seed g = dL/dlogits of this trial ----------------
        float gs[NCLS];
        if (kind == EEGNET_SEED_DLOGITS) {
#pragma unroll
            for (int n = 0; n < NCLS; ++n) gs[n] = dlog[(size_t)b * NCLS + n];
        } else {
            float l[NCLS];
#pragma unroll
            for (int n = 0; n < NCLS; ++n) l[n] = Lg[n];
            int cls = 0;
            if (tgt) {
                cls = (int)tgt[b];
            } else {                                       // the trial's own argmax, lowest index on a tie
                float best = l[0];
#pragma unroll
                for (int n = 1; n < NCLS; ++n)
                    if (l[n] > best) { best = l[n]; cls = n; }
            }
            if (kind == EEGNET_SEED_LOGIT) {
#pragma unroll
                for (int n = 0; n < NCLS; ++n) gs[n] = n == cls ? 1.f : 0.f;
            } else {                                       // softmax(logits) - onehot(target)
                float ex[NCLS], mx;
                const float sum = softmax4(l, ex, mx);
#pragma unroll
                for (int n = 0; n < NCLS; ++n) gs[n] = ex[n] / sum - (n == cls ? 1.f : 0.f);
            }
        }
        // ---------------- backward ----------------
        if (row_on) {
            // dr[o,t] = s3 dh[o,t/8]/8 ELU'(z3[o,t]), dh = Wfc^T g; over the d2 row (its last reader was
            // this wave's depthwise FIR)
            float* drw = D2s + o * RS2 + LP2;
            const float* wfc = prm + g.o_Wfc + o * T2;
#pragma unroll
            for (int m = 0; m < MAXT1Q; ++m) {
                const int t = lane + 64 * m;
                if (t < T1) {
                    float v = 0.f;
                    if (t < 8 * T2) {
                        float dh = 0.f;
#pragma unroll
                        for (int n = 0; n < NCLS; ++n) dh = fmaf(wfc[n * NF + (t >> 3)], gs[n], dh);
                        v = w.s3 * 0.125f * dh * elu_d(fmaf(w.s3, r[m], w.b3));
                    }
                    drw[t] = v;
                }
            }
        }
        __syncthreads();                                   // dr rows complete; the q rows are free
        if (row_on) {
            float dq[MAXT1Q];
            w3t_rows(prm + g.o_W3 + o, F2, T1, RS2, D2s + LP2, lane, dq);
            row_store(Qs + o * RS2 + LP2, T1, lane, dq);   // dq over the q row
            wave_lds_fence();
            // al dz2[4q + i] = dd2[q] (al/4 ELU'), over the s row
            const float* qb = Qs + o * RS2 + (LP2 + 7);
            float* srow = Ss + o * RS + LP;
            const float* erow = Es + o * RS + LP;
            for (int q = lane; q < T1; q += 64) {
                const float a = fir16_t(w.w2, qb, q);
                const floatx4 e = lds_ld4(erow + 4 * q);
                lds_st4(srow + 4 * q, (floatx4){a * e[0], a * e[1], a * e[2], a * e[3]});
            }
            // the samples pool4 drops (t >= 4 T1) get no gradient from z2, but their ds is not zero
            for (int t = 4 * T1 + lane; t < T; t += 64) srow[t] = 0.f;
            wave_lds_fence();
            temporal_row_t<K1>(Ss + o * RS, Es + o * RS + LP, T, TQ, w.tap, tapl, lane);     // ds over the ELU' row
        }
        __syncthreads();                                   // ds rows complete
        // dx[c,t] = sum_o ws[o,c] ds[o,t]: v_mfma_f32_16x16x4_f32, A = ws^T (registers), B = ds tile
        // (4 o x 16 t), D[4 (l >> 4) + r][l & 15] -> the x rows (their reader was this trial's spatial GEMM)
        for (int n = wave; n < NT16; n += NWAVE) {
            float bv[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) bv[s] = 4 * s + lk < F2 ? Es[(4 * s + lk) * RS + LP + 16 * n + li] : 0.f;
            const int t = 16 * n + li;
#pragma unroll
            for (int ct = 0; ct < NCTM; ++ct) {
                if (ct < NCT) {
                    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (4 * s < F2) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(awT[ct][s], bv[s], acc, 0, 0, 0);
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        const int c = 16 * ct + 4 * lk + rr;
                        if (c < C && t < T) Xs[c * RS + LP + t] = acc[rr];
                    }
                }
            }
        }
        __syncthreads();                                   // dx rows staged
        // dx[b] is C*T contiguous floats: whole rows, consecutive lanes on consecutive addresses; 16-byte
        // stores only when every row starts 16-byte aligned (T % 4 == 0 and an aligned dx: `vec`)
        {
            float* dxb = dx + (size_t)b * nx;
            if (vec) {
                const int nq = (C * T) >> 2, TQ4 = T >> 2;
                for (int i = tid; i < nq; i += NTH) {
                    const int c = i / TQ4, q = i - c * TQ4;
                    const floatx4 v = lds_ld4(Xs + c * RS + LP + 4 * q);
                    *reinterpret_cast<floatx4*>(dxb + 4 * (size_t)i) = v;
                }
            } else {
                for (int i = tid; i < C * T; i += NTH) {
                    const int c = i / T, t = i - c * T;
                    dxb[i] = Xs[c * RS + LP + t];
                }
            }
        }
        __syncthreads();                                   // dx rows read: the next trial's x may land
        if (bnx < g.B) x_store<PF>(pf, C, T, RS, LP, Xs, tid);
        __syncthreads();
    }
}

}  // namespace eeg
