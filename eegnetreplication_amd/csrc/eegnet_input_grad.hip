// eegnet_input_grad.hip -- eval-mode input gradients (saliency): the fused forward + dL/dx kernel
// behind eegnet_input_grad_eval.  Included by eegnet_kernels.hip (one translation unit).
//
// In eval mode BatchNorm is affine with the running statistics and there is no dropout, so every trial
// is independent and dx is the transposed chain of what k_infer computes:
//     forward   s = ws x;  v = FIR_w1(s);  z2 = al v + be;  d2 = pool4(ELU(z2));  q = FIR_w2(d2);
//               r = W3 q;  z3 = s3 r + b3;  h = pool8(ELU(z3));  logits = Wfc h + bfc
//     backward  dh = Wfc^T g;  dr = s3 dh/8 ELU'(z3);  dq = W3^T dr;  dd2 = FIR^T_w2(dq);
//               dz2 = dd2/4 ELU'(z2);  ds = FIR^T_w1(al dz2);  dx = ws^T ds
// k_infer_dx has k_infer's shape: 1024 threads, wave o owns row o of every [F2, T] plane, one workgroup
// per trial in flight, trials strided over the grid, the next trial's x prefetched into registers.  A
// trial never leaves the CU between x and dx.  LDS (floats, make_geo's ldsX):
//     Xs [C][RS]     x rows; after the spatial GEMM has read them, the staging rows of dx
//     Ss [F2][RS]    s rows; then al dz2 (the operand of the transposed temporal FIR)
//     Es [F2][RS]    al/4 ELU'(z2); then ds (the B operand of the dx GEMM)
//     D2s [F2][RS2]  d2 rows (left pad LP2); then dr
//     Qs [F2][RS2]   q rows (left pad LP2); then dq
//     Hs [NF], Lg [4]
// ELU'(z3) is recomputed from r, which a lane still holds in registers when the seed arrives.  The pads
// of every padded row are zeroed once and never written, so nothing of a trial (a NaN included) reaches
// the next one.

namespace eeg {

template <int K1, int CC, int TT, int FF>
__global__ __launch_bounds__(NTH) void k_infer_dx(Geo g, const float* __restrict__ prm,
                                                  const float* __restrict__ bn, const float* __restrict__ x,
                                                  int kind, const float* __restrict__ dlog,
                                                  const int64_t* __restrict__ tgt, float* __restrict__ dx,
                                                  float* __restrict__ logits, int vec) {
    using G_ = KG<K1>;
    EEG_DIMS(g);
    constexpr int NCTM = CC ? (CC + 15) / 16 : 4;      // 16-channel tiles of the dx GEMM (C <= 64)
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* const Xs = sm;
    float* const Ss = Xs + C * RS;
    float* const Es = Ss + F2 * RS;
    float* const D2s = Es + F2 * RS;
    float* const Qs = D2s + F2 * RS2;
    float* const Hs = Qs + F2 * RS2;
    float* const Lg = Hs + ((NF + 3) & ~3);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const float* rm1 = bn;                 const float* rv1 = bn + g.F1;
    const float* rm2 = bn + 2 * g.F1;      const float* rv2 = rm2 + F2;
    const float* rm3 = rm2 + 2 * F2;       const float* rv3 = rm3 + F2;

    for (int i = tid; i < (C + 2 * F2) * RS + 2 * F2 * RS2; i += NTH) sm[i] = 0.f;
    float aw[KS];
    load_ws_frag<KS>(prm + g.o_ws, C, F2, aw, lane);
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
    float tap[K1];
#pragma unroll
    for (int k = 0; k < K1; ++k) tap[k] = prm[g.o_w1 + gg * K1 + k];
    const float tapl = lane < K1 ? prm[g.o_w1 + gg * K1 + lane] : 0.f;     // tap `lane` (the ds tail samples)
    float w2[K2], w3[F2MAX];
#pragma unroll
    for (int k = 0; k < K2; ++k) w2[k] = prm[g.o_w2 + oo * K2 + k];
#pragma unroll
    for (int i = 0; i < F2MAX; ++i) w3[i] = i < F2 ? prm[g.o_W3 + oo * F2 + i] : 0.f;
    // eval BN1 and BN2 folded: z2 = al * v + be; BN3: z3 = s3 r + b3 (as k_infer)
    float al, be, s3, b3;
    {
        const float a1 = prm[g.o_g1 + gg] / sqrtf(rv1[gg] + g.eps);
        const float c1 = prm[g.o_b1 + gg] - a1 * rm1[gg];
        float W = 0.f;
        for (int c = 0; c < C; ++c) W += prm[g.o_ws + oo * C + c];
        const float s2 = prm[g.o_g2 + oo] / sqrtf(rv2[oo] + g.eps);
        al = a1 * s2;
        be = (c1 * W - rm2[oo]) * s2 + prm[g.o_b2 + oo];
        s3 = prm[g.o_g3 + oo] / sqrtf(rv3[oo] + g.eps);
        b3 = prm[g.o_b3 + oo] - rm3[oo] * s3;
    }
    const float al4 = 0.25f * al;
    const size_t nx = (size_t)C * T;
    float pf[PF];
    if ((int)blockIdx.x < g.B) x_prefetch<PF>(x + (size_t)blockIdx.x * nx, C, T, pf, tid);
    __syncthreads();
    x_store<PF>(pf, C, T, RS, LP, Xs, tid);
    __syncthreads();
    drain_prologue_loads();

    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        const int bnx = b + gridDim.x;
        if (bnx < g.B) x_prefetch<PF>(x + (size_t)bnx * nx, C, T, pf, tid);
        // ---------------- forward ----------------
        spatial_mfma<KS>(Xs, aw, Ss, C, F2, NT16, RS, LP, wave, lane);
        __syncthreads();                                   // s rows complete; the x rows are free
        if (row_on) {
            const float* row = Ss + o * RS;
            float* erow = Es + o * RS + LP;
            float* drow = D2s + o * RS2 + LP2;
            for (int q = lane; q < T1; q += 64) {
                float w[4 * G_::NW];
                lds_window<G_::NW>(row + 4 * q, w);
                float v[4];
                fir4<K1, G_::OFF>(w, tap, v);
                float pe = 0.f;
                floatx4 e;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float z = fmaf(al, v[i], be), ez = fast_exp(z);
                    pe += z > 0.f ? z : ez - 1.f;
                    e[i] = z > 0.f ? al4 : al4 * ez;       // al/4 ELU'(z2)
                }
                drow[q] = pe * 0.25f;
                lds_st4(erow + 4 * q, e);
            }
            wave_lds_fence();
            // block_2 depthwise: q[t] = sum_k w2[k] d2[t + k - 7]
            const float* dr = D2s + o * RS2 + 1;
            float* qrow = Qs + o * RS2 + LP2;
#pragma unroll
            for (int m = 0; m < MAXT1Q; ++m) {
                const int t = lane + 64 * m;
                if (t < T1) {
                    float a = 0.f;
#pragma unroll
                    for (int k = 0; k < K2; ++k) a = fmaf(w2[k], dr[t + k], a);
                    qrow[t] = a;
                }
            }
        }
        __syncthreads();                                   // q rows complete
        float r[MAXT1Q];
#pragma unroll
        for (int m = 0; m < MAXT1Q; ++m) {
            const int t = lane + 64 * m;
            float a = 0.f;
            if (row_on && t < T1) {
#pragma unroll
                for (int i = 0; i < F2MAX; ++i)
                    if (i < F2) a = fmaf(w3[i], Qs[i * RS2 + LP2 + t], a);
            }
            r[m] = a;
        }
#pragma unroll
        for (int m = 0; m < MAXT1Q; ++m) {
            const int t = lane + 64 * m;
            float e = (row_on && t < 8 * T2) ? elu_f(fmaf(s3, r[m], b3)) : 0.f;
            e += dpp<0xB1>(e);                 // 8-lane sums by DPP (xor 1, xor 2, half-row mirror)
            e += dpp<0x4E>(e);
            e += dpp<0x141>(e);
            if (row_on && (t & 7) == 0 && t < 8 * T2) Hs[o * T2 + (t >> 3)] = e * 0.125f;
        }
        __syncthreads();                                   // h complete
        if (wave < NCLS) {
            const int n = wave;
            float a = 0.f;
            for (int i = lane; i < NF; i += 64) a = fmaf(prm[g.o_Wfc + n * NF + i], Hs[i], a);
            a = wave_sum(a);
            if (lane == 0) {
                const float l = a + prm[g.o_bfc + n];
                Lg[n] = l;
                if (logits) logits[(size_t)b * NCLS + n] = l;
            }
        }
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
                const float mx = fmaxf(fmaxf(l[0], l[1]), fmaxf(l[2], l[3]));
                float ex[NCLS], sum = 0.f;
#pragma unroll
                for (int n = 0; n < NCLS; ++n) { ex[n] = expf(l[n] - mx); sum += ex[n]; }
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
                        v = s3 * 0.125f * dh * elu_d(fmaf(s3, r[m], b3));
                    }
                    drw[t] = v;
                }
            }
        }
        __syncthreads();                                   // dr rows complete; the q rows are free
        if (row_on) {
            // dq[o,t] = sum_i W3[i,o] dr[i,t] over the q row
            float* qrow = Qs + o * RS2 + LP2;
            const float* w3c = prm + g.o_W3 + o;
#pragma unroll
            for (int m = 0; m < MAXT1Q; ++m) {
                const int t = lane + 64 * m;
                if (t < T1) {
                    float a = 0.f;
#pragma unroll
                    for (int i = 0; i < F2MAX; ++i)
                        if (i < F2) a = fmaf(w3c[i * F2], D2s[i * RS2 + LP2 + t], a);
                    qrow[t] = a;
                }
            }
            wave_lds_fence();
            // dd2[q] = sum_k w2[k] dq[q - k + 7] (pads swapped: 8 | 7); al dz2[4q + i] = dd2[q] (al/4 ELU')
            const float* qb = Qs + o * RS2 + (LP2 + 7);
            float* srow = Ss + o * RS + LP;
            const float* erow = Es + o * RS + LP;
            for (int q = lane; q < T1; q += 64) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < K2; ++k) a = fmaf(w2[k], qb[q - k], a);
                const floatx4 e = lds_ld4(erow + 4 * q);
                lds_st4(srow + 4 * q, (floatx4){a * e[0], a * e[1], a * e[2], a * e[3]});
            }
            // the samples pool4 drops (t >= 4 T1) get no gradient from z2, but their ds is not zero
            for (int t = 4 * T1 + lane; t < T; t += 64) srow[t] = 0.f;
            wave_lds_fence();
            // ds[t] = sum_k w1[k] (al dz2)[t - k + P]: the forward FIR with the taps flipped, pads R | P
            const float* row = Ss + o * RS;
            float* dsrow = Es + o * RS + LP;
            // One or two quads past a multiple of 64 (22 x 257: quad 64 holds the one sample t = 256) would
            // cost a whole window pass with one or two lanes on: the lane-parallel loop stops at NQF and
            // those samples are 64-lane dot products instead, lane k on tap k
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
