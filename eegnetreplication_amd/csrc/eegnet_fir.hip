// eegnet_fir.hip -- FIR filtering of continuous recordings: the reference's zero-phase band-pass
// (raw.filter(4., 38., fir_design='firwin'), dataset.py:113-125) for any taps, whole recordings and recordings
// fed block by block.  Behind eegnet_fir; included by eegnet_kernels.hip (one translation unit).
//
// Per row, with taps h[0..L-1] and M = (L-1)/2, output sample t is
//     y[t] = sum_{k = 0..L-1} h[k] u[t + M - k]
// added in the order k = 0, 1, .., L-1 by one fp64 fused multiply-add per tap from a zero start, and rounded
// to fp32 once.  u is the row extended past its ends (fir_ext): by mne's 'reflect_limited' rule at an end of
// the recording -- u[-j] = 2 x[0] - x[j], u[n-1+j] = 2 x[n-1] - x[n-1-j] for j up to min(M, n-1), zero
// beyond -- or, for a block in the middle of a stream, by the L-1 samples before it kept as fp64 history.
// A value of u is a function of at most two input samples (2 x is exact, the difference rounds once), so an
// output is a fixed function of the taps and of its L values of u whatever chunk, thread, row count, pitch
// or call it falls into: a stream's concatenated output carries the bits of the whole-recording call.
//
// One workgroup per (row, chunk of FIR_CH outputs): it stages the chunk's FIR_CH + L - 1 values of u into
// LDS as fp64, then every thread runs FIR_S consecutive outputs over a sliding register window -- one LDS
// read and FIR_S FMAs per tap, the tap wave-uniform (scalar loads).  The LDS rows are skewed by one double
// per FIR_S so that the threads' reads, FIR_S doubles apart, fall into different banks.  Outputs leave
// through LDS, so that a wave stores consecutive floats.  No atomics, no workgroup waits on another.
// k_fir_hist writes the stream's next history (the last L-1 samples of history + block) to a second buffer.

namespace eeg {

constexpr int FIR_NT = 256;                   // threads of a chunk's workgroup
constexpr int FIR_S = 8;                      // consecutive outputs of a thread
constexpr int FIR_CH = FIR_NT * FIR_S;        // outputs of a chunk (eegnet_fir_chunk)
constexpr int FIR_MAX_TAPS = 2049;            // eegnet_fir_max_taps: a 0.5 Hz transition at 250 Hz is 1651 taps

struct FirCall {
    long long n_rows, n, n_out, n_chunks;     // rows, input samples per row, outputs per row, chunks per row
    long long x_pitch, y_pitch;               // elements between rows
    long long t_lo;                           // output o is sample t_lo + o of the block's time axis
    long long refl;                           // samples an end is reflected over: min(M, recording's length - 1)
    int L, M;
    int head_reflect, tail_reflect;           // the block's left / right end is the recording's
};

// LDS position of staged element i (one double of skew per FIR_S)
__device__ __forceinline__ int fir_skew(int i) { return i + (i >> 3); }
static_assert(FIR_S == 8, "fir_skew and the window rotation are written for 8 outputs per thread");

// doubles of LDS of a chunk's workgroup: elements 0 .. FIR_CH + L - 1 (element 0 is a pad that is read
// with the last tap and never used), skewed; not less than the FIR_CH floats the outputs leave through
static inline int fir_lds_doubles(int L) {
    const int last = FIR_CH + L - 1;
    return last + (last >> 3) + 1;
}

// sample g of the row as the call sees it: the block for 0 <= g < n, the history (hr, nullable) for
// -(L-1) <= g < 0, else 0.  Nothing outside the block or the history is read.
template <class T>
__device__ __forceinline__ double fir_val(const FirCall& fc, const T* __restrict__ xr, const double* __restrict__ hr,
                                          long long g) {
    if (g >= 0) return g < fc.n ? (double)xr[g] : 0.0;
    const long long i = g + fc.L - 1;
    return (hr != nullptr && i >= 0) ? hr[i] : 0.0;
}

// u[g]: the row extended past the block's ends
template <class T>
__device__ __forceinline__ double fir_ext(const FirCall& fc, const T* __restrict__ xr, const double* __restrict__ hr,
                                          long long g) {
    if (g < 0 && fc.head_reflect) {
        const long long j = -g;
        return j <= fc.refl ? 2.0 * fir_val(fc, xr, hr, 0) - fir_val(fc, xr, hr, j) : 0.0;
    }
    if (g >= fc.n) {
        if (!fc.tail_reflect) return 0.0;
        const long long j = g - (fc.n - 1);
        return j <= fc.refl ? 2.0 * fir_val(fc, xr, hr, fc.n - 1) - fir_val(fc, xr, hr, fc.n - 1 - j) : 0.0;
    }
    return fir_val(fc, xr, hr, g);
}

// grid: n_rows * n_chunks workgroups, row-major.  hist_in [n_rows][L-1] (nullable: no history).
// dynamic LDS: fir_lds_doubles(L) doubles.
template <class T>
__global__ __launch_bounds__(FIR_NT) void k_fir(FirCall fc, const T* __restrict__ x, const double* __restrict__ h,
                                                const double* __restrict__ hist_in, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) double fir_e[];
    const int tid = threadIdx.x;
    const int L = fc.L;
    const long long row = (long long)blockIdx.x / fc.n_chunks, j = (long long)blockIdx.x - row * fc.n_chunks;
    const long long c0 = j * FIR_CH;                                  // the chunk's first output
    const int nloc = (int)(fc.n_out - c0 < FIR_CH ? fc.n_out - c0 : FIR_CH);
    const T* xr = x ? x + row * fc.x_pitch : nullptr;
    const double* hr = hist_in ? hist_in + row * (long long)(L - 1) : nullptr;

    // element i >= 1 is u[g0 + i - 1], g0 the sample the chunk's first output meets its last tap at
    const long long g0 = fc.t_lo + c0 + fc.M - (L - 1);
    const int n_stage = FIR_CH + L;
    for (int i = tid; i < n_stage; i += FIR_NT)
        fir_e[fir_skew(i)] = i == 0 ? 0.0 : fir_ext(fc, xr, hr, g0 + i - 1);
    __syncthreads();

    // output o of the chunk: sum_k h[k] e[o + L - k].  w[s] of tap k is e[base + s - k]; from one tap to the
    // next the window moves down by one element, so the registers rotate: at step u of an unrolled group
    // of FIR_S taps w[s] lives in r[(s - u) & 7] and the element that enters replaces the one that left.
    const int base = tid * FIR_S + L;
    double r[FIR_S], acc[FIR_S];
#pragma unroll
    for (int s = 0; s < FIR_S; ++s) {
        r[s] = fir_e[fir_skew(base + s)];
        acc[s] = 0.0;
    }
    int k = 0;
    for (; k + FIR_S <= L; k += FIR_S) {
#pragma unroll
        for (int u = 0; u < FIR_S; ++u) {
            const double hk = h[k + u];
#pragma unroll
            for (int s = 0; s < FIR_S; ++s) acc[s] = fma(hk, r[(s - u) & 7], acc[s]);
            r[(7 - u) & 7] = fir_e[fir_skew(base - 1 - (k + u))];
        }
    }
#pragma unroll
    for (int u = 0; u < FIR_S - 1; ++u) {
        if (k + u < L) {
            const double hk = h[k + u];
#pragma unroll
            for (int s = 0; s < FIR_S; ++s) acc[s] = fma(hk, r[(s - u) & 7], acc[s]);
            r[(7 - u) & 7] = fir_e[fir_skew(base - 1 - (k + u))];
        }
    }

    // through LDS (every thread is past its last read of e), then consecutive floats per wave
    __syncthreads();
    float* ys = reinterpret_cast<float*>(fir_e);
#pragma unroll
    for (int s = 0; s < FIR_S; ++s) ys[tid * FIR_S + s] = (float)acc[s];
    __syncthreads();
    float* yc = y + row * fc.y_pitch + c0;
    for (int o = tid; o < nloc; o += FIR_NT) yc[o] = ys[o];
}

// grid: ceil(n_rows (L-1) / FIR_NT) workgroups.  hist_out[row][i] = sample n - (L-1) + i of history + block.
template <class T>
__global__ __launch_bounds__(FIR_NT) void k_fir_hist(FirCall fc, const T* __restrict__ x,
                                                     const double* __restrict__ hist_in, double* __restrict__ hist_out) {
    const long long H = fc.L - 1;
    const long long idx = (long long)blockIdx.x * FIR_NT + threadIdx.x;
    if (idx >= fc.n_rows * H) return;
    const long long row = idx / H, i = idx - row * H;
    const T* xr = x ? x + row * fc.x_pitch : nullptr;
    const double* hr = hist_in ? hist_in + row * H : nullptr;
    hist_out[idx] = fir_val(fc, xr, hr, fc.n - H + i);
}

}  // namespace eeg
