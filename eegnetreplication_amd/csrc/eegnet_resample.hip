// eegnet_resample.hip -- rational polyphase resampling up/down of continuous recordings (scipy's
// resample_poly, mne's method="polyphase"; NOT the FFT method that the reference's raw.resample(128,
// npad="auto"), dataset.py:114, defaults to), whole recordings and recordings fed block by block.  Behind
// eegnet_resample; included by eegnet_kernels.hip (one translation unit).
//
// Per row, with the prototype taps h[0..L-1], L = 2 half + 1, up and down coprime, output m is, with
// c = m down + half,
//     y[m] = sum_{n = ceil((c - 2 half) / up) .. floor(c / up)} h[c - n up] u[n]
// added in the order of ascending tap index c - n up (descending n) by one fp64 fused multiply-add per term
// from a zero start, and rounded to fp32 once.  With p = c mod up (the output's phase) and q = floor(c / up)
// the terms are h[p + j up] u[q - j], j = 0, 1, ..: the taps of one phase lie up apart, so the prototype padded
// with zeros to K up entries, K = ceil(L / up), IS the table [j][p] of K rows of up phases, and every output
// runs exactly K terms.  A padded term adds 0 * u to the sum, which leaves a finite sum's value as it is; the
// one thing it can change is the sign of a zero: a sum that is exactly -0.0 (every product before it -0.0 or
// underflowed to it) becomes +0.0 when 0 * u is +0.0, and u there lies outside the output's support.  The two
// compare equal; "the same bits" below is meant up to the sign of an exact zero.
//
// u is the row extended past its ends (rs_ext): by zeros, or by the band-pass's odd reflection --
// u[-j] = 2 x[0] - x[j], u[N-1+j] = 2 x[N-1] - x[N-1-j] for j up to min(Q + 1, N - 1), Q = half / up, zero
// beyond (no output reaches further than Q + 1 samples past an end) -- or, for a block in the middle of a
// stream, by the H = 2 Q + 2 values of u before it kept as fp64 history (the history of a stream's first
// block holds the head's reflected values, so a continuation never reflects).  A value of u is a function
// of at most two input samples (2 x is exact, the difference rounds once), so an output is a fixed function
// of the taps and of the K values of u in its support whatever chunk, thread, row count, pitch or call it
// falls into: a stream's concatenated output carries the bits of the whole-recording call.
//
// One workgroup per row and group of up to RS_CPW consecutive chunks of rc.ch outputs (the host sizes ch so
// that the table and a chunk's input span fit the LDS of the launch, and the group so that the launch keeps
// RS_MIN_GRID workgroups).  It stages the table once, then per chunk the span -- u[q(first output) - (K-1)] ..
// u[q(last output)] -- as fp64, and thread t runs the outputs t, t + RS_NT, .. of the chunk: lanes own
// consecutive outputs, so a wave's stores are consecutive floats without a pass through LDS, the phases of
// a half-wave's 32 lanes step by down mod up (coprime to up: distinct table columns), and when up divides
// RS_NT the outputs of one thread share their phase, so one table read serves RS_S of them.  No atomics, no
// workgroup waits on another.  k_resample_hist writes the stream's next history to a second buffer.

namespace eeg {

constexpr int RS_NT = 256;                    // threads of a chunk's workgroup
constexpr int RS_S = 4;                       // outputs of a thread, RS_NT apart
constexpr int RS_CH = RS_NT * RS_S;           // the most outputs of a chunk
constexpr int RS_CPW = 8;                     // the most chunks of a workgroup (one staged table serves them)
constexpr int RS_MIN_GRID = 2048;             // workgroups a launch keeps before a workgroup takes a second chunk
constexpr int RS_MAX_TAPS = 4097;             // eegnet_resample_max_taps: 250 -> 128 Hz is 2501, 160/147 is 3201
constexpr int RS_MAX_UP = 256;                // eegnet_resample_max_up
constexpr int RS_MAX_DOWN = 1 << 20;          // (a chunk's offsets from its first output stay in 32 bits)

struct RsCall {
    long long n_rows, n, n_out, n_chunks;     // rows, input samples per row, outputs per row, chunks per row
    long long x_pitch, y_pitch;               // elements between rows
    long long t0;                             // the recording's sample index of the block's first sample
    long long m_lo;                           // the recording's output index of the call's first output
    long long refl;                           // samples an end is reflected over: min(Q + 1, recording's length - 1)
    int L, half, up, down;
    long long n_groups;                       // workgroups per row
    int K, H, ch, cpw;                        // terms of an output; history per row; outputs of a chunk; chunks of a workgroup
    int head_ext, tail_ext;                   // the block's left / right end is the recording's
    int reflect;                              // the ends are reflected (else zero)
    int share;                                // up divides RS_NT: a thread's outputs have one phase
};

// doubles of the input span a chunk of ch outputs stages at most: q moves by at most
// floor((ch - 1) down / up) + 1 over the chunk, and the first output reaches K - 1 below its q
static inline long long rs_span_doubles(long long ch, int up, int down, int K) {
    return (ch - 1) * (long long)down / up + 1 + K;
}

// sample g of the recording as the call sees it: the block for t0 <= g < t0 + n, the history (hr, nullable)
// for t0 - H <= g < t0, else 0.  Nothing outside the block or the history is read.
template <class T>
__device__ __forceinline__ double rs_val(const RsCall& rc, const T* __restrict__ xr, const double* __restrict__ hr,
                                         long long g) {
    const long long b = g - rc.t0;
    if (b >= 0) return b < rc.n ? (double)xr[b] : 0.0;
    const long long i = b + rc.H;
    return (hr != nullptr && i >= 0) ? hr[i] : 0.0;
}

// u[g]: the recording extended past its ends
template <class T>
__device__ __forceinline__ double rs_ext(const RsCall& rc, const T* __restrict__ xr, const double* __restrict__ hr,
                                         long long g) {
    if (g < 0 && rc.head_ext) {
        const long long j = -g;
        return rc.reflect && j <= rc.refl ? 2.0 * rs_val(rc, xr, hr, 0) - rs_val(rc, xr, hr, j) : 0.0;
    }
    const long long last = rc.t0 + rc.n - 1;
    if (g > last) {
        if (!rc.tail_ext) return 0.0;
        const long long j = g - last;
        return rc.reflect && j <= rc.refl ? 2.0 * rs_val(rc, xr, hr, last) - rs_val(rc, xr, hr, last - j) : 0.0;
    }
    return rs_val(rc, xr, hr, g);
}

// the K terms of a thread's RS_S outputs: tab + p[s] is the phase's column, e + b[s] the sample at its q
template <bool SHARE>
__device__ __forceinline__ void rs_terms(const double* __restrict__ tab, const double* __restrict__ e, int up, int K,
                                         const int (&p)[RS_S], const int (&b)[RS_S], double (&acc)[RS_S]) {
#pragma unroll 4
    for (int j = 0; j < K; ++j) {
        const double h0 = tab[j * up + p[0]];
#pragma unroll
        for (int s = 0; s < RS_S; ++s) {
            const double hs = SHARE ? h0 : tab[j * up + p[s]];
            acc[s] = fma(hs, e[b[s] - j], acc[s]);
        }
    }
}

// chunk ck of a row: its span staged in e, then the outputs.  The table is staged; the workgroup is in step.
template <class T>
__device__ __forceinline__ void rs_chunk(const RsCall& rc, long long ck, const T* __restrict__ xr,
                                         const double* __restrict__ hr, const double* __restrict__ tab,
                                         double* __restrict__ e, float* __restrict__ yr) {
    const int tid = threadIdx.x;
    const int up = rc.up, down = rc.down, K = rc.K;
    const long long c0 = ck * rc.ch;                                  // the chunk's first output of the call
    const int nloc = (int)(rc.n_out - c0 < rc.ch ? rc.n_out - c0 : rc.ch);

    // the chunk's first output is output m0 of the recording, at c = m0 down + half = q0 up + p0; output o
    // of the chunk is at q0 up + p0 + o down (the offset fits 32 bits: o < RS_CH, down <= RS_MAX_DOWN)
    const long long cc = (rc.m_lo + c0) * down + rc.half;
    const long long q0 = cc / up;
    const int p0 = (int)(cc - q0 * up);
    const long long g0 = q0 - (K - 1);                                // the first staged sample: e[i] = u[g0 + i]
    const int n_stage = (p0 + (nloc - 1) * down) / up + K;
    const long long lo = g0 - rc.t0;                                  // the span's place in the block
    if (lo >= 0 && lo + n_stage <= rc.n) {                            // inside it: the samples as they lie
        const T* xs = xr + lo;
        for (int i = tid; i < n_stage; i += RS_NT) e[i] = (double)xs[i];
    } else {
        for (int i = tid; i < n_stage; i += RS_NT) e[i] = rs_ext(rc, xr, hr, g0 + i);
    }
    __syncthreads();

    int p[RS_S], b[RS_S];
    double acc[RS_S];
#pragma unroll
    for (int s = 0; s < RS_S; ++s) {
        const int o = tid + s * RS_NT;
        const int r = p0 + (o < nloc ? o : 0) * down;                 // (an idle slot reruns output 0)
        const int q = r / up;
        p[s] = r - q * up;
        b[s] = q + K - 1;
        acc[s] = 0.0;
    }
    if (rc.share) rs_terms<true>(tab, e, up, K, p, b, acc);
    else rs_terms<false>(tab, e, up, K, p, b, acc);
#pragma unroll
    for (int s = 0; s < RS_S; ++s) {
        const int o = tid + s * RS_NT;
        if (o < nloc) yr[c0 + o] = (float)acc[s];
    }
    __syncthreads();                                                  // (the next chunk's span replaces this one)
}

// grid: n_rows * n_groups workgroups, row-major.  hist_in [n_rows][H] (nullable: no history).
// dynamic LDS: K up + rs_span_doubles(ch) doubles.
template <class T>
__global__ __launch_bounds__(RS_NT) void k_resample(RsCall rc, const T* __restrict__ x, const double* __restrict__ h,
                                                    const double* __restrict__ hist_in, float* __restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) double rs_lds[];
    const long long row = (long long)blockIdx.x / rc.n_groups, grp = (long long)blockIdx.x - row * rc.n_groups;
    const T* xr = x ? x + row * rc.x_pitch : nullptr;
    const double* hr = hist_in ? hist_in + row * (long long)rc.H : nullptr;
    double* tab = rs_lds;                                             // [K][up]: the prototype, zero-padded
    const int n_tab = rc.K * rc.up;
    for (int i = threadIdx.x; i < n_tab; i += RS_NT) tab[i] = i < rc.L ? h[i] : 0.0;
    const long long ck_end = (grp + 1) * rc.cpw < rc.n_chunks ? (grp + 1) * rc.cpw : rc.n_chunks;
    for (long long ck = grp * rc.cpw; ck < ck_end; ++ck)
        rs_chunk(rc, ck, xr, hr, tab, rs_lds + n_tab, y + row * rc.y_pitch);
}

// grid: ceil(n_rows H / RS_NT) workgroups.  hist_out[row][i] = u[t0 + n - H + i] of history + block.
template <class T>
__global__ __launch_bounds__(RS_NT) void k_resample_hist(RsCall rc, const T* __restrict__ x,
                                                         const double* __restrict__ hist_in, double* __restrict__ hist_out) {
    const long long H = rc.H;
    const long long idx = (long long)blockIdx.x * RS_NT + threadIdx.x;
    if (idx >= rc.n_rows * H) return;
    const long long row = idx / H, i = idx - row * H;
    const T* xr = x ? x + row * rc.x_pitch : nullptr;
    const double* hr = hist_in ? hist_in + row * H : nullptr;
    hist_out[idx] = rs_ext(rc, xr, hr, rc.t0 + rc.n - H + i);
}

}  // namespace eeg
