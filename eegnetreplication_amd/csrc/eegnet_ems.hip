// eegnet_ems.hip -- exponential moving standardisation of continuous recordings (the reference's
// raw_exponential_moving_standardize, dataset.py:45-70) as a blocked scan over time.  Behind eegnet_ems;
// included by eegnet_kernels.hip (one translation unit).
//
// Per channel row, with a = factor_new, p = 1 - a and (m, v) carried from sample to sample:
//     m_t = p m_{t-1} + a x_t,   v_t = p v_{t-1} + a (x_t - m_t)^2,   y_t = (x_t - m_t) / sqrt(v_t + eps)
// Both recurrences are first order and linear with the constant coefficient p, so they are scans.  Time is
// cut into chunks of EMS_L samples; a workgroup owns one (row, chunk), a thread EMS_S consecutive samples.
// Three launches, ordered by the stream and by nothing else:
//   k_ems_agg    every chunk's aggregates from a zero start: with r the chunk's first sample, loc the local
//                mean scan of x - r and e = x - r - loc, the chunk's last loc (A), the last value of the scan
//                S0 of a e^2 and the sum E of e.  With c = m_in - r the mean the chunk is entered with,
//                m_k = r + loc_k + c p^(k+1), so (x_k - m_k)^2 = e_k^2 - 2 c e_k p^(k+1) + c^2 p^(2k+2) and
//                the variance scan splits into three scans that do not know c:
//                    v_k = p^(k+1) v_in + S0_k - 2 c a p^(k+1) E_k + c^2 p^(k+2) (1 - p^(k+1))
//                (the p^(k-j) of the scan and the p^(j+1) of the middle term multiply to p^(k+1), which leaves
//                a plain sum; the last term is a geometric series).  Taking r off first keeps c at the size
//                of the signal's deviation, not of its DC offset: nothing large cancels.
//   k_ems_carry  one wave per row: the initial (m, v) -- a two-pass fp64 reduction over the first
//                min(init_block, n) samples, or the state handed in -- then lane 0 walks the row's chunk
//                aggregates in order, leaves the (m, v) each chunk is entered with, and writes the final state.
//   k_ems_out    the scans again per chunk, now from the true carries: m directly, then v of the true
//                (x - m)^2, then y, rounded to fp32 once.  It reads its chunk into registers before it writes,
//                and no other workgroup touches that chunk, so y may be x.
// All arithmetic is fp64.  No workgroup waits on another and there are no atomics: the same inputs give the
// same bits.  Powers of p come from repeated products (ems_powi), never from pow().

namespace eeg {

constexpr int EMS_NT = 256;                   // threads of a chunk's workgroup
constexpr int EMS_NW = EMS_NT / 64;           // its waves
constexpr int EMS_S = 8;                      // consecutive samples of a thread
constexpr int EMS_L = EMS_NT * EMS_S;         // samples of a chunk (eegnet_ems_chunk)
constexpr int EMS_AGG = 4;                    // doubles of a chunk's aggregates: r, A, S0, E
constexpr int EMS_NTC = 64;                   // threads of k_ems_carry: one wave per row

struct EmsCall {
    long long n_rows, n, n_chunks;            // rows, samples per row, chunks per row
    long long x_pitch, y_pitch;               // elements between rows
    double a, p, eps;                         // factor_new, 1 - factor_new, eps
    long long init_n;                         // min(init_block, n); unused when resuming
    int resume;
};

// b^e by squaring: products only
__device__ __forceinline__ double ems_powi(double b, unsigned long long e) {
    double r = 1.0;
    while (e) {
        if (e & 1ull) r *= b;
        b *= b;
        e >>= 1;
    }
    return r;
}

// The powers a chunk's thread needs, of q = p^EMS_S: one thread's segment.
struct EmsPow {
    double qd[7];            // q^(2^i): the strides of the wave scan, and q^64 across waves
    double qlane;            // q^lane
    double qtid;             // q^tid = p^(EMS_S tid): from the chunk's entry to this thread's first sample
};

__device__ __forceinline__ EmsPow ems_pow(double p, int tid) {
    EmsPow w;
    w.qd[0] = ems_powi(p, EMS_S);
#pragma unroll
    for (int i = 1; i < 7; ++i) w.qd[i] = w.qd[i - 1] * w.qd[i - 1];
    w.qlane = ems_powi(w.qd[0], (unsigned)(tid & 63));
    w.qtid = w.qlane * ems_powi(w.qd[6], (unsigned)(tid >> 6));
    return w;
}

// Exclusive scan over the workgroup's threads of s_i = q s_{i-1} + val_i from s_{-1} = 0: returns s_{i-1},
// the value thread i's segment is entered with.  qd[i] = q^(2^i), qlane = q^lane; all ones for a plain
// sum.  Inside a wave by __shfl_up, across the waves through `lds` (EMS_NW doubles, this call's own:
// one barrier).
__device__ __forceinline__ double ems_scan_excl(double val, const double (&qd)[7], double qlane, double* lds,
                                                int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    double s = val;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const double t = __shfl_up(s, 1u << i);
        if (lane >= (1 << i)) s += qd[i] * t;
    }
    if (lane == 63) lds[wave] = s;
    __syncthreads();
    double win = 0.0;
    for (int u = 0; u < wave; ++u) win = qd[6] * win + lds[u];
    double ex = __shfl_up(s, 1u);
    if (lane == 0) ex = 0.0;
    return ex + win * qlane;
}

// A thread's samples of chunk `xc` (nloc valid samples), less r; 0 past the row's end, where nothing is read.
// A full chunk takes its EMS_S consecutive elements unguarded, so the compiler may merge them into 16-byte
// loads (gfx950 takes those at 4-byte alignment).
template <class T>
__device__ __forceinline__ void ems_load(const T* xc, int nloc, double r, int tid, double (&xs)[EMS_S]) {
    if (nloc == EMS_L) {
#pragma unroll
        for (int s = 0; s < EMS_S; ++s) xs[s] = (double)xc[tid * EMS_S + s] - r;
    } else {
#pragma unroll
        for (int s = 0; s < EMS_S; ++s) {
            const int k = tid * EMS_S + s;
            xs[s] = k < nloc ? (double)xc[k] - r : 0.0;
        }
    }
}

// grid: n_rows * n_chunks workgroups, row-major.  agg [n_rows][n_chunks][EMS_AGG].
template <class T>
__global__ __launch_bounds__(EMS_NT) void k_ems_agg(EmsCall ec, const T* __restrict__ x, double* __restrict__ agg) {
    __shared__ double sh[3 * EMS_NW];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x / ec.n_chunks, j = (long long)blockIdx.x - row * ec.n_chunks;
    const long long t0 = j * EMS_L;
    const int nloc = (int)(ec.n - t0 < EMS_L ? ec.n - t0 : EMS_L);
    const T* xc = x + row * ec.x_pitch + t0;
    const double a = ec.a, p = ec.p;
    const EmsPow w = ems_pow(p, tid);
    const double ones[7] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0};
    const double r = (double)xc[0];
    double xs[EMS_S];
    ems_load(xc, nloc, r, tid, xs);

    double l = 0.0;
#pragma unroll
    for (int s = 0; s < EMS_S; ++s) l = p * l + a * xs[s];
    const double l_in = ems_scan_excl(l, w.qd, w.qlane, sh, tid);

    double e[EMS_S], s0 = 0.0, es = 0.0;
    l = l_in;
#pragma unroll
    for (int s = 0; s < EMS_S; ++s) {
        l = p * l + a * xs[s];
        e[s] = xs[s] - l;
        s0 = p * s0 + a * e[s] * e[s];
        es += e[s];
    }
    const double s0_in = ems_scan_excl(s0, w.qd, w.qlane, sh + EMS_NW, tid);
    const double es_in = ems_scan_excl(es, ones, 1.0, sh + 2 * EMS_NW, tid);

    // the thread that holds the chunk's last valid sample runs its segment up to it and writes the aggregates
    const int last = nloc - 1 - tid * EMS_S;
    if (last >= 0 && last < EMS_S) {
        l = l_in;
        s0 = s0_in;
        es = es_in;
#pragma unroll
        for (int s = 0; s < EMS_S; ++s) {
            if (s <= last) {
                l = p * l + a * xs[s];
                s0 = p * s0 + a * e[s] * e[s];
                es += e[s];
            }
        }
        double* o = agg + (size_t)blockIdx.x * EMS_AGG;
        o[0] = r;
        o[1] = l;
        o[2] = s0;
        o[3] = es;
    }
}

// sum over the wave of a lane's value, in a fixed order; every lane gets it
__device__ __forceinline__ double ems_wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// grid: n_rows workgroups of one wave.  carry [n_rows][n_chunks][2] = the (m, v) a chunk is entered with;
// state [n_rows][2] (nullable): read when resuming, written with the final (m, v).
template <class T>
__global__ __launch_bounds__(EMS_NTC) void k_ems_carry(EmsCall ec, const T* __restrict__ x,
                                                       const double* __restrict__ agg, double* __restrict__ carry,
                                                       double* state) {
    const int lane = threadIdx.x;
    const long long row = blockIdx.x;
    double m, v;
    if (ec.resume) {
        m = state[2 * row];
        v = state[2 * row + 1];
    } else {
        // mean, then the population variance about it: each lane adds its samples in index order, the
        // lanes' sums meet in a fixed butterfly
        const T* xr = x + row * ec.x_pitch;
        double sum = 0.0;
        for (long long i = lane; i < ec.init_n; i += EMS_NTC) sum += (double)xr[i];
        m = ems_wave_sum(sum) / (double)ec.init_n;
        double sq = 0.0;
        for (long long i = lane; i < ec.init_n; i += EMS_NTC) {
            const double d = (double)xr[i] - m;
            sq += d * d;
        }
        v = ems_wave_sum(sq) / (double)ec.init_n;
    }
    if (lane != 0) return;
    const double a = ec.a, p = ec.p;
    const double p_full = ems_powi(p, EMS_L);
    const double p_last = ems_powi(p, (unsigned long long)(ec.n - (ec.n_chunks - 1) * EMS_L));
    const double* ag = agg + (size_t)row * ec.n_chunks * EMS_AGG;
    double* cr = carry + (size_t)row * ec.n_chunks * 2;
#pragma unroll 4
    for (long long j = 0; j < ec.n_chunks; ++j) {
        const double r = ag[EMS_AGG * j], A = ag[EMS_AGG * j + 1], S0 = ag[EMS_AGG * j + 2], E = ag[EMS_AGG * j + 3];
        cr[2 * j] = m;
        cr[2 * j + 1] = v;
        const double pn = j + 1 < ec.n_chunks ? p_full : p_last;      // p^(the chunk's samples)
        const double c = m - r;
        m = r + A + c * pn;
        v = pn * (v - 2.0 * c * a * E + c * c * p * (1.0 - pn)) + S0;
    }
    if (state) {
        state[2 * row] = m;
        state[2 * row + 1] = v;
    }
}

// grid: as k_ems_agg.  y may be x (fp32): a chunk is in registers before its first store.
template <class T>
__global__ __launch_bounds__(EMS_NT) void k_ems_out(EmsCall ec, const T* x, const double* __restrict__ carry, float* y) {
    __shared__ double sh[2 * EMS_NW];
    const int tid = threadIdx.x;
    const long long row = (long long)blockIdx.x / ec.n_chunks, j = (long long)blockIdx.x - row * ec.n_chunks;
    const long long t0 = j * EMS_L;
    const int nloc = (int)(ec.n - t0 < EMS_L ? ec.n - t0 : EMS_L);
    const T* xc = x + row * ec.x_pitch + t0;
    float* yc = y + row * ec.y_pitch + t0;
    const double a = ec.a, p = ec.p;
    const EmsPow w = ems_pow(p, tid);
    const double r = (double)xc[0];
    double xs[EMS_S];
    ems_load(xc, nloc, r, tid, xs);
    const double c = carry[(size_t)blockIdx.x * 2] - r, v_chunk = carry[(size_t)blockIdx.x * 2 + 1];

    double l = 0.0;
#pragma unroll
    for (int s = 0; s < EMS_S; ++s) l = p * l + a * xs[s];
    const double l_in = ems_scan_excl(l, w.qd, w.qlane, sh, tid) + c * w.qtid;

    double d[EMS_S], vs = 0.0;
    l = l_in;
#pragma unroll
    for (int s = 0; s < EMS_S; ++s) {
        l = p * l + a * xs[s];
        d[s] = xs[s] - l;                                  // x - m: r leaves both
        vs = p * vs + a * d[s] * d[s];
    }
    double v = ems_scan_excl(vs, w.qd, w.qlane, sh + EMS_NW, tid) + v_chunk * w.qtid;
    float ys[EMS_S];
#pragma unroll
    for (int s = 0; s < EMS_S; ++s) {
        v = p * v + a * d[s] * d[s];
        ys[s] = (float)(d[s] / sqrt(v + ec.eps));
    }
    // every thread is past both scans' barriers, so every load of the chunk, xc[0] included, is done
    if (nloc == EMS_L) {
#pragma unroll
        for (int s = 0; s < EMS_S; ++s) yc[tid * EMS_S + s] = ys[s];
    } else {
#pragma unroll
        for (int s = 0; s < EMS_S; ++s) {
            const int k = tid * EMS_S + s;
            if (k < nloc) yc[k] = ys[s];
        }
    }
}

}  // namespace eeg
