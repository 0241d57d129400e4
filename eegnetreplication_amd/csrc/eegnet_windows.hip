// eegnet_windows.hip -- sliding-window inference over continuous recordings, read in place: the eval
// forward of every T-sample window of a recording (k_infer_win) and the crop-averaged class
// probabilities / prediction per recording (k_win_reduce).  Behind eegnet_forward_eval_windows; included
// by eegnet_kernels.hip (one translation unit).
//
// A recording is C channel rows of n_samples floats, `pitch` floats apart; window w of it is samples
// [w hop, w hop + T) of each row.  k_infer_win is k_infer with another loader: win_prefetch fills the
// pf registers x_prefetch would fill from that window copied out as a [C][T] trial, x_store writes the
// same LDS rows, and the trial body is the forward of eegnet_trial.hip's pieces in infer_trial's order --
// so logits[r, w] carries the bits eegnet_forward_eval gives for the copy.  infer_trial itself is not
// called: it fetches the next trial through x_prefetch, and it stays as it is (eegnet_trial.hip's header).
//
// eegnet_forward_eval_windows_at runs the same kernel with the window origin read from a table (cue
// epoching in place): k_infer_win's second variant, on a WinAtCall, takes window p from sample starts[p] of
// recording rec_index[p], both clamped into the recordings, and picks the load width per window.
//
// Overlapping windows share nothing: the 'same' padding makes a window's first and last FIR outputs its
// own, the pool4 phase follows hop mod 4, and a shared block 1 would not be bit-equal to k_infer.

namespace eeg {

struct WinCall {
    const float* rec;             // row (r, c) at rec + (r C + c) pitch
    long long pitch;              // floats between channel rows (>= n_samples)
    long long hop;                // samples between window starts
    int W;                        // windows per recording
    int total;                    // n_rec * W: logits rows
    int vec;                      // every window row starts 16-byte aligned: float4 loads
};

// sample 0 of row 0 of window p = r W + w (wave-uniform)
__device__ __forceinline__ const float* win_row0(const WinCall& wc, int C, int p) {
    const int r = p / wc.W, w = p - r * wc.W;
    return wc.rec + (long long)r * C * wc.pitch + (long long)w * wc.hop;
}

// The windows of a table: window p is samples [starts[p], starts[p] + T) of recording rec_index[p]
// (nullable: recording 0).  `total` is the table's length; hop, W and vec are unused.
struct WinAtCall : WinCall {
    const long long* starts;      // [total], device
    const int* rec_index;         // [total], device, nullable
    long long last;               // n_samples - T: the largest start
    int n_rec;
};

// where window p starts and whether its rows take 16-byte loads (both wave-uniform)
struct WinOrg {
    const float* row0;
    int vec;
};

__device__ __forceinline__ WinOrg win_org(const WinCall& wc, int C, int, int p) { return {win_row0(wc, C, p), wc.vec}; }

// A start is clamped into [0, last] and a recording index into [0, n_rec): whatever the table holds, every
// load lies inside the recordings.
__device__ __forceinline__ WinOrg win_org(const WinAtCall& ac, int C, int T, int p) {
    long long st = ac.starts[p];
    st = st < 0 ? 0 : st > ac.last ? ac.last : st;
    int r = ac.rec_index ? ac.rec_index[p] : 0;
    r = r < 0 ? 0 : r >= ac.n_rec ? ac.n_rec - 1 : r;
    const float* row0 = ac.rec + (long long)r * C * ac.pitch + st;
    const int vec = (T & 3) == 0 && (ac.pitch & 3) == 0 && (reinterpret_cast<uintptr_t>(row0) & 15) == 0;
    return {row0, vec};
}

// x_prefetch of a window: element i of the flattened [C][T] window is sample i % T of row i / T.  The
// register layout is x_prefetch's (quads when T % 4 == 0), whichever load width fetches it; every load
// lies in [0, T) of its row.
template <int PF>
__device__ __forceinline__ void win_prefetch(const float* __restrict__ xb, long long pitch, int vec, int C, int T,
                                             float (&pf)[PF], int tid) {
    const int n = C * T;
    if ((T & 3) == 0) {
        const int TQ = T >> 2;
#pragma unroll
        for (int j = 0; j < PF / 4; ++j) {
            const int i = tid + NTH * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * i < n) {
                const int c = i / TQ, q = i - c * TQ;
                const float* src = xb + c * pitch + 4 * q;
                if (vec) {
                    v = *reinterpret_cast<const float4*>(src);
                } else {
                    // four 4-byte loads of one quad: the compiler may issue them as one 16-byte load at
                    // 4-byte alignment, which gfx950 takes (unaligned global access is on by default)
                    v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
                }
            }
            pf[4 * j] = v.x; pf[4 * j + 1] = v.y; pf[4 * j + 2] = v.z; pf[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int i = tid + NTH * j;
            float v = 0.f;
            if (i < n) {
                const int c = i / T, t = i - c * T;
                v = xb[c * pitch + t];
            }
            pf[j] = v;
        }
    }
}

// One 1024-thread workgroup per window in flight, windows strided over a flat grid (k_infer's for
// B = n_rec W).  The next window's load is issued at the top of a trial and stored over the x rows
// behind their last reader, the spatial GEMM.
template <int K1, int CC, int TT, int FF, class Call = WinCall>
__global__ __launch_bounds__(NTH) void k_infer_win(Geo g, const float* __restrict__ prm,
                                                   const float* __restrict__ bn, Call wc,
                                                   float* __restrict__ logits) {
    EEG_DIMS(g);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const TrialLds L = trial_lds(C, F2, RS, RS2, NF, false);
    float* const Xs = sm;
    float* const Ss = sm + L.Ss;
    float* const D2s = sm + L.D2s;
    float* const Qs = sm + L.Qs;
    float* const Hs = sm + L.Hs;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    for (int i = tid; i < L.Hs; i += NTH) sm[i] = 0.f;
    InferOps<K1, KS> w;
    infer_ops_load<K1, CC, TT, FF, false>(g, prm, bn, wave, lane, w);
    const int o = wave;
    const bool row_on = o < F2;
    float pf[PF];
    if ((int)blockIdx.x < wc.total) {
        const WinOrg org = win_org(wc, C, T, blockIdx.x);
        win_prefetch<PF>(org.row0, wc.pitch, org.vec, C, T, pf, tid);
    }
    __syncthreads();
    x_store<PF>(pf, C, T, RS, LP, Xs, tid);
    __syncthreads();
    drain_prologue_loads();

    for (int b = blockIdx.x; b < wc.total; b += gridDim.x) {
        const int bnx = b + gridDim.x;
        const bool nxt = bnx < wc.total;
        if (nxt) {
            const WinOrg org = win_org(wc, C, T, bnx);
            win_prefetch<PF>(org.row0, wc.pitch, org.vec, C, T, pf, tid);
        }
        spatial_mfma<KS>(Xs, w.aw, Ss, C, F2, NT16, RS, LP, wave, lane);
        __syncthreads();                                   // s rows complete; the x rows are free
        if (row_on)
            temporal_row<K1>(Ss + o * RS, D2s + o * RS2 + LP2, T1, w.tap, lane,
                             [&](int, const float (&v)[4]) { return elu_pool4(w.al, w.be, v); });
        if (nxt) x_store<PF>(pf, C, T, RS, LP, Xs, tid);
        __syncthreads();
        float r[MAXT1Q];
        block2_rows(F2, T1, RS2, D2s, Qs, w.w2, w.w3, row_on, o, lane, r);
        pool8_head(T2, Hs, w.s3, w.b3, r, row_on, o, lane, [](int) { return 1.f; });
        __syncthreads();                                   // h complete
        classifier(g, prm, Hs, NF, wave, lane, [&](int n, float l) { logits[(size_t)b * NCLS + n] = l; });
        __syncthreads();
    }
}

// One workgroup per recording: probs[r] = mean_w softmax(logits[r, w]) and pred[r] = its argmax, the
// lowest index on a tie.  Thread j adds the fp64 softmax of windows j, j + NTWR, ... in index order,
// thread 0 adds the NTWR partials in thread order and divides by W.  A function of the logits alone: the
// same inputs give the same bits.
constexpr int NTWR = 256;
__global__ __launch_bounds__(NTWR) void k_win_reduce(const float* __restrict__ logits, int W,
                                                     float* __restrict__ probs, int32_t* __restrict__ pred) {
    __shared__ double sh[NTWR][NCLS];
    const int tid = threadIdx.x;
    const float* lr = logits + (size_t)blockIdx.x * W * NCLS;
    double acc[NCLS] = {0.0, 0.0, 0.0, 0.0};
    for (int wi = tid; wi < W; wi += NTWR) {
        double l[NCLS], ex[NCLS];
#pragma unroll
        for (int n = 0; n < NCLS; ++n) l[n] = (double)lr[(size_t)wi * NCLS + n];
        const double mx = fmax(fmax(l[0], l[1]), fmax(l[2], l[3]));
        double sum = 0.0;
#pragma unroll
        for (int n = 0; n < NCLS; ++n) { ex[n] = exp(l[n] - mx); sum += ex[n]; }
#pragma unroll
        for (int n = 0; n < NCLS; ++n) acc[n] += ex[n] / sum;
    }
#pragma unroll
    for (int n = 0; n < NCLS; ++n) sh[tid][n] = acc[n];
    __syncthreads();
    if (tid == 0) {
        double m[NCLS] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < NTWR; ++j)
#pragma unroll
            for (int n = 0; n < NCLS; ++n) m[n] += sh[j][n];
#pragma unroll
        for (int n = 0; n < NCLS; ++n) m[n] /= (double)W;
        int cls = 0;
        double best = m[0];
#pragma unroll
        for (int n = 1; n < NCLS; ++n)
            if (m[n] > best) { best = m[n]; cls = n; }
        if (probs) {
#pragma unroll
            for (int n = 0; n < NCLS; ++n) probs[(size_t)blockIdx.x * NCLS + n] = (float)m[n];
        }
        if (pred) pred[blockIdx.x] = cls;
    }
}

}  // namespace eeg
