// Does a cache-policy modifier on a streamed load or store keep its lines out of the Infinity Cache?
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/ic_policy_probe tools/ic_policy_probe.hip && tools/ic_policy_probe
//
// A table of TABLE_MB is read once (it then sits in the 256 MiB Infinity Cache), STREAM_MB of other memory is
// streamed past it under one policy, and the table is read again under the plain policy and timed.  If the
// stream's lines were allocated in the cache, table + stream exceed it and the re-read comes from HBM; if the
// policy keeps them out, the re-read is as fast as with no stream in between.  Two fixed points frame the
// answers: no stream at all (all hits) and a plain stream of twice the cache (all misses).  Prints the median
// and the range of REPS re-reads per policy, in microseconds and TB/s.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef float floatx4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

enum Pol { PLAIN, NT, SC1, SC0SC1, SC0SC1NT, ST_PLAIN, ST_NT, NPOL };
static const char* kName[NPOL] = {"load plain", "load nt", "load sc1", "load sc0 sc1", "load sc0 sc1 nt",
                                  "store plain", "store nt"};

template <int P>
__device__ __forceinline__ floatx4 ld(const floatx4* p) {
    floatx4 v;
    if constexpr (P == PLAIN) v = *p;
    else if constexpr (P == NT) v = __builtin_nontemporal_load(p);
    else if constexpr (P == SC1) asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    else if constexpr (P == SC0SC1) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    else asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1 nt\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// n4 float4s, grid-stride; every thread's sum goes to out[thread] so that no load is dropped
template <int P>
__global__ void k_read(const floatx4* __restrict__ src, size_t n4, float* __restrict__ out) {
    const size_t nth = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    for (size_t i = t; i < n4; i += nth) acc += ld<P>(src + i);
    out[t] = acc[0] + acc[1] + acc[2] + acc[3];
}
template <bool NTS>
__global__ void k_write(floatx4* __restrict__ dst, size_t n4) {
    const size_t nth = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const floatx4 v = {1.f, 2.f, 3.f, 4.f};
    for (size_t i = t; i < n4; i += nth) {
        if constexpr (NTS) __builtin_nontemporal_store(v, dst + i);
        else dst[i] = v;
    }
}

int main(int argc, char** argv) {
    const size_t TABLE_MB = argc > 1 ? atoi(argv[1]) : 160, STREAM_MB = argc > 2 ? atoi(argv[2]) : 200;
    const int REPS = 7, GRID = 2048, NT_ = 256;
    const size_t tn4 = TABLE_MB * 1000000 / 16, sn4 = STREAM_MB * 1000000 / 16, bigger = std::max(sn4, (size_t)540 * 1000000 / 16);
    floatx4 *table, *stream;
    float* out;
    CK(hipMalloc(&table, tn4 * 16));
    CK(hipMalloc(&stream, bigger * 16));
    CK(hipMalloc(&out, (size_t)GRID * NT_ * 4));
    CK(hipMemset(table, 0, tn4 * 16));
    CK(hipMemset(stream, 0, bigger * 16));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto run_stream = [&](int pol, size_t n4) {
        switch (pol) {
        case PLAIN: k_read<PLAIN><<<GRID, NT_>>>(stream, n4, out); break;
        case NT: k_read<NT><<<GRID, NT_>>>(stream, n4, out); break;
        case SC1: k_read<SC1><<<GRID, NT_>>>(stream, n4, out); break;
        case SC0SC1: k_read<SC0SC1><<<GRID, NT_>>>(stream, n4, out); break;
        case SC0SC1NT: k_read<SC0SC1NT><<<GRID, NT_>>>(stream, n4, out); break;
        case ST_PLAIN: k_write<false><<<GRID, NT_>>>(stream, n4); break;
        case ST_NT: k_write<true><<<GRID, NT_>>>(stream, n4); break;
        }
    };
    auto measure = [&](const char* name, int pol, size_t n4) {
        std::vector<float> us;
        for (int r = 0; r < REPS; ++r) {
            k_read<PLAIN><<<GRID, NT_>>>(table, tn4, out);          // the table into the cache
            if (pol >= 0) run_stream(pol, n4);
            CK(hipEventRecord(e0));
            k_read<PLAIN><<<GRID, NT_>>>(table, tn4, out);          // the timed re-read
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            us.push_back(1e3f * ms);
        }
        std::sort(us.begin(), us.end());
        const double by = (double)tn4 * 16;
        printf("%-28s re-read of %zu MB: median %7.1f us (%5.2f TB/s), range %7.1f - %7.1f us\n", name, TABLE_MB,
               us[REPS / 2], by / us[REPS / 2] * 1e-6, us.front(), us.back());
    };
    printf("table %zu MB, stream %zu MB, Infinity Cache 268 MB\n", TABLE_MB, STREAM_MB);
    measure("no stream (all hits)", -1, 0);
    measure("plain load stream of 540 MB", PLAIN, bigger);
    for (int p = 0; p < NPOL; ++p) measure(kName[p], p, sn4);
    CK(hipDeviceSynchronize());
    return 0;
}
