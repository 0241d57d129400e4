// eegnet_eval_folds.hip -- fold-indexed validation: the eval forward, per-trial cross-entropy and argmax
// of every resident fold's model on its own held-out set in one launch (k_eval_folds), and the
// reference's validation loss / correct count per fold in a second (k_eval_folds_reduce).  Behind
// eegnet_eval_folds; included by eegnet_kernels.hip (one translation unit).
//
// The reference validates after every epoch (model.py:151-172): per DataLoader batch of `batch` trials
// the mean CE, then running / len(loader), and the count of argmax == label.  In eval mode every trial
// is independent, so k_eval_folds is k_infer's per-trial body (infer_trial, eegnet_trial.hip) with the
// model taken from a device table of eegnet_eval_fold records.
//
// Grid: flat.  The (fold, trial) pairs are laid out as nfolds rows of max_n slots, pair p = fold * max_n
// + trial, and workgroup w of G <= CU count walks the contiguous range [w chunk, (w + 1) chunk); slots
// at or past a fold's own n are skipped.  When its range crosses into another fold the workgroup reads
// that fold's record and rebuilds the per-fold operands (infer_ops_load).  k_infer is one 1024-thread
// workgroup per CU, so a (workgroups per fold, fold) grid of 90 folds either leaves 76 CUs idle (2 per
// fold) or runs a second dispatch round of 14 workgroups (3 per fold); the flat grid gives every CU
// total / G trials whatever the fold count.  A trial's result does not depend on which workgroup runs
// it (no arithmetic crosses trials), so the split is free to follow the launch width.
//
// No atomics, no tickets, no workgroup waits on another: logits / ce / pred are per-trial stores, and
// the reduction (one workgroup per fold, stream-ordered behind the first kernel) sums in a fixed order.

namespace eeg {

struct EvalCall {
    const eegnet_eval_fold* folds;
    long long max_n;              // slots per fold in the pair layout (>= every fold's n)
    long long total;              // nfolds * max_n
    long long chunk;              // pairs per workgroup
    long long slot;               // loss / correct slot
    int batch;                    // trials per batch mean of the validation loss
};

// fold `i`'s record through the constant address space (as fold_rec): a scalar load, and the pointers
// in it are known to be global
__device__ __forceinline__ eegnet_eval_fold eval_rec(const eegnet_eval_fold* folds, long long i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(4))) eegnet_eval_fold*)folds)[i];
#else
    return folds[i];                               // (the host pass of a device function)
#endif
}

// per-trial cross-entropy logsumexp(l) - l[y] (pass C's formulation) and argmax, lowest index on a tie
__device__ __forceinline__ float ce_of_logits(const float (&l)[NCLS], int y) {
    float ex[NCLS], mx;
    const float se = softmax4(l, ex, mx);
    const float lse = mx + logf(se);
    const float ly = y == 0 ? l[0] : y == 1 ? l[1] : y == 2 ? l[2] : l[3];
    return lse - ly;
}
__device__ __forceinline__ int argmax_of_logits(const float (&l)[NCLS]) {
    int cls = 0;
    float best = l[0];
#pragma unroll
    for (int n = 1; n < NCLS; ++n)
        if (l[n] > best) { best = l[n]; cls = n; }
    return cls;
}

template <int K1, int CC, int TT, int FF>
__global__ __launch_bounds__(NTH) void k_eval_folds(Geo g, EvalCall ec) {
    EEG_DIMS(g);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* const Lg = sm + (C + F2) * RS + 2 * F2 * RS2 + ((NF + 3) & ~3);     // the trial's logits
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t nx = (size_t)C * T;

    // the rows' pads are zeroed once and never written: every fold has the same row geometry
    for (int i = tid; i < (C + F2) * RS + 2 * F2 * RS2; i += NTH) sm[i] = 0.f;
    const long long p1 = min(((long long)blockIdx.x + 1) * ec.chunk, ec.total);
    long long p = (long long)blockIdx.x * ec.chunk;
    float pf[PF];
    while (p < p1) {
        const long long fold = p / ec.max_n, t0 = p - fold * ec.max_n;
        const long long tend = min(ec.max_n, t0 + (p1 - p));
        p += tend - t0;
        const eegnet_eval_fold f = eval_rec(ec.folds, fold);
        const long long t1 = min(tend, (long long)f.n);
        if (t0 >= t1) continue;                     // this fold's own trials end before the range
        const float* const prm = f.params;
        InferOps<K1, KS> w;
        infer_ops_load<K1, CC, TT, FF, true>(g, prm, f.bn_buffers, wave, lane, w);
        x_prefetch<PF>(f.x + (size_t)t0 * nx, C, T, pf, tid);
        __syncthreads();                            // the pads are zero; the previous fold's readers are done
        x_store<PF>(pf, C, T, RS, LP, sm, tid);
        __syncthreads();
        drain_prologue_loads();
        for (long long b = t0; b < t1; ++b) {
            const float* xn = b + 1 < t1 ? f.x + (size_t)(b + 1) * nx : nullptr;
            // the label is wave-uniform and never written here: a scalar load, issued a trial ahead of its use
            const int y = f.labels ? (int)ldc(f.labels + b) : 0;
            infer_trial<K1, CC, TT, FF>(g, prm, w, sm, xn, pf, tid, wave, lane, [&](int n, float l) {
                if (f.logits) f.logits[(size_t)b * NCLS + n] = l;
                Lg[n] = l;
            });
            // the trial's last barrier is behind us: Lg holds its logits, and the next write to it comes
            // three barriers into the next trial
            if (tid == 0) {
                float l[NCLS];
#pragma unroll
                for (int n = 0; n < NCLS; ++n) l[n] = Lg[n];
                if (f.labels && f.ce) f.ce[b] = ce_of_logits(l, y);
                if (f.pred) f.pred[b] = argmax_of_logits(l);
            }
        }
    }
}

// One workgroup per fold.  Thread j sums batch j, j + NTER, ... of the fold's ce in fp64 and index order
// (the last batch may be short), divides by the batch's size and adds the mean to its own partial; thread
// 0 then adds the NTER partials in thread order and divides by the number of batches: the reference's
// running_val_loss / len(val_loader).  The correct count is an integer sum.  A function of ce / pred /
// labels alone: the same inputs give the same bits.
constexpr int NTER = 256;
__global__ __launch_bounds__(NTER) void k_eval_folds_reduce(EvalCall ec) {
    __shared__ double shl[NTER];
    __shared__ long long shc[NTER];
    const eegnet_eval_fold f = eval_rec(ec.folds, blockIdx.x);
    // no labels, no sums -- but an empty fold (whose labels pointer may well be NULL) still reports 0 / 0
    if ((!f.labels && f.n > 0) || (!f.loss && !f.correct)) return;      // (uniform: the workgroup leaves)
    const int tid = threadIdx.x;
    const long long n = f.n, nb = (n + ec.batch - 1) / ec.batch;
    double part = 0.0;
    long long cnt = 0;
    if (f.loss)
        for (long long j = tid; j < nb; j += NTER) {
            const long long i0 = j * ec.batch, i1 = min(i0 + ec.batch, n);
            double s = 0.0;
            for (long long i = i0; i < i1; ++i) s += (double)f.ce[i];
            part += s / (double)(i1 - i0);
        }
    if (f.correct)
        for (long long i = tid; i < n; i += NTER) cnt += (long long)f.pred[i] == (long long)f.labels[i] ? 1 : 0;
    shl[tid] = part;
    shc[tid] = cnt;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        long long c = 0;
        for (int j = 0; j < NTER; ++j) { s += shl[j]; c += shc[j]; }
        if (f.loss) f.loss[ec.slot] = nb > 0 ? s / (double)nb : 0.0;
        if (f.correct) f.correct[ec.slot] = (int64_t)c;
    }
}

}  // namespace eeg
