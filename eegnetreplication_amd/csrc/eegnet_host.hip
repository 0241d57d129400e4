// eegnet_host.hip -- host side of libeegnet_hip.so: geometry/validation, workspace layout, launch
// sequences of the train step and the C-ABI of include/eegnet_abi.h.  Included by eegnet_kernels.hip.
// ================================================================================================
// Host side: geometry, validation, launch sequences, C-ABI.
// ================================================================================================
using namespace eeg;

static thread_local std::string g_err;

static int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

static inline size_t rupz(size_t a, size_t m) { return (a + m - 1) / m * m; }

constexpr size_t CNT_BYTES = (size_t)TK_COUNT * NCNT * TKS * 4;     // a multiple of 16

static int device_cus() {
    static int cus = 0;
    if (cus == 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;     // MI355X
    }
    return cus;
}

static unsigned long long* g_trace_buf = nullptr;     // eegnet_trace_enable

// The shipped library reads no environment: kernel choice and grids are functions of the dims alone.
// The F2 <= 16 step runs passes C / D as k_pass_c (one trial per wave) and k_pass_dr (the row-layout
// kernel on the streaming grid, eegnet_passes.hip).  The build switches that once selected other
// variants -- round 5's one-trial-per-wave pass D, 256-thread whole-trial passes C / D, grid
// multipliers, the whole-trial bf16 eval kernel at cfg5 -- lost their measurements
// and are gone; commit d0e7be7 is the last that contains them.

// the dims every entry point takes; nothing is computed from dims that fail here
static int check_dims(const eegnet_dims* d) {
    if (!d) return fail(EEGNET_EINVAL, "dims is NULL");
    const int F2 = d->F1 * d->D;
    if (d->B < 1) return fail(EEGNET_EINVAL, "B must be >= 1 (got %d)", d->B);
    if (d->K1 != 32 && d->K1 != 64) return fail(EEGNET_EINVAL, "K1 must be 32 or 64 (got %d)", d->K1);
    if (d->C < 1 || d->C > 64) return fail(EEGNET_EINVAL, "C must be in [1,64] (got %d)", d->C);
    if (d->F1 < 1 || d->D < 1 || F2 > 64 || (F2 & 3))
        return fail(EEGNET_EINVAL, "F1*D must be a multiple of 4 in [4,64] (got F1=%d D=%d)", d->F1, d->D);
    if (d->T < 32 || d->T < d->K1 || d->T > 1024)
        return fail(EEGNET_EINVAL, "T must be in [max(32,K1), 1024] (got %d)", d->T);
    const int XP = d->x_pitch ? d->x_pitch : d->T;
    if (XP != d->T && !(x_pitch_shape(model_dims(*d)) && (XP & 3) == 0 && XP > d->T))
        return fail(EEGNET_EINVAL, "x_pitch %d: only the 22 x 257 EEGNet-8,2 (K1 = 32) training kernels take "
                    "a row pitch, a multiple of 4 above T (eegnet_x_pitch)", XP);
    if (!(d->p_drop >= 0.f && d->p_drop <= 1.f)) return fail(EEGNET_EINVAL, "p_drop must be in [0,1]");
    if (F2 * (d->T / 32) < 1) return fail(EEGNET_EINVAL, "T//32 must be >= 1");
    return 0;
}

// what the launches of a geometry's kernels can take: prefetch registers, per-thread tables, 32-bit
// indices, LDS
static int check_launch(const Geo& g) {
    if (g.wide) {
        if (g.C > 4 * KSW) return fail(EEGNET_EINVAL, "C = %d > %d", g.C, 4 * KSW);
        if (g.T1 > 16 * NTTW * (NWB2 / 4)) return fail(EEGNET_EINVAL, "T/4 = %d > %d", g.T1, 16 * NTTW * (NWB2 / 4));
        if (g.NF > MAXNFW * NTB2) return fail(EEGNET_EINVAL, "F2*(T/32) = %d > %d", g.NF, MAXNFW * NTB2);
        if ((double)g.B * g.F2 * g.T1 >= 4294967296.0)
            return fail(EEGNET_EINVAL, "B*F2*(T/4) must stay below 2^32 (dropout / mask indices)");
    } else {
        if (g.C * g.T > NTH * MAXPF)
            return fail(EEGNET_EINVAL, "C*T = %d exceeds the %d-float prefetch of one trial", g.C * g.T, NTH * MAXPF);
        if (g.T1 > 64 * MAXT1Q) return fail(EEGNET_EINVAL, "T/4 > %d", 64 * MAXT1Q);
        if (g.F2 * g.T1 > 4 * NTH) return fail(EEGNET_EINVAL, "F2*(T/4) > %d", 4 * NTH);
        if ((double)g.B * g.F2 * g.T1 >= 4294967296.0)
            return fail(EEGNET_EINVAL, "B*F2*(T/4) must stay below 2^32 (dropout / mask indices)");
        if (g.NF > 64 * MAXNFQ) return fail(EEGNET_EINVAL, "F2*(T/32) = %d > %d", g.NF, 64 * MAXNFQ);
        if (g.nparam > APT * NTB) return fail(EEGNET_EINVAL, "%d parameters > %d", g.nparam, APT * NTB);
    }
    const int lmax = g.wide ? std::max({g.ldsWA, g.ldsWB, g.ldsWB2, g.ldsWC, g.ldsWD, g.ldsWE, g.ldsWI})
                            : std::max({g.ldsA, g.ldsB, g.ldsC, g.ldsD, g.ldsE, g.ldsI});
    if (lmax * 4 > LDS_MAX) return fail(EEGNET_EINVAL, "dims need %d B of LDS (> %d)", lmax * 4, LDS_MAX);
    return 0;
}

// Geometry of a call: the dims checked, the shape fields by geo_shape (eegnet_geometry.h: the function the
// compile-time geometries are values of), then what the call and the device add -- the batch, the dropout
// and BatchNorm arguments, the grids -- and, with `launch`, the launch limits.
static int make_geo(const eegnet_dims* d, Geo* g, bool launch = true) {
    if (int r = check_dims(d)) return r;
    *g = geo_shape(model_dims(*d));
    g->trace = g_trace_buf;
    g->B = g->Bn = d->B;
    g->XP = d->x_pitch ? d->x_pitch : g->T;
    g->p = d->p_drop; g->eps = d->bn_eps; g->mom = d->bn_momentum;
    g->scale = g->p < 1.f ? 1.f / (1.f - g->p) : 0.f;
    const int cus = device_cus();
    g->grid = std::min(g->B, cus);                      // pass C, the block-2 passes, the eval forward
    if (g->wide) {
        // streaming grid: one 1024-thread workgroup per CU, NOC per trial range; a multiple of 8 * NOC
        // when it can be (the chunk workgroups of a range then share an XCD)
        int G = std::min(g->B * g->NOC, cus);
        G = std::max(g->NOC, G / g->NOC * g->NOC);
        if (G >= 8 * g->NOC) G = G / (8 * g->NOC) * (8 * g->NOC);
        g->gridS = G;
        // cfg5: two 8-wave workgroups of k_wpass_b2 / c per CU, two trials each at B = 1024, so one
        // workgroup's barriers overlap the other's work
        g->gridW2 = is_cfg5(model_dims(*g)) ? std::min(g->B, 2 * cus) : g->grid;
    } else {
        g->gridS = std::min(g->B, cus * WGPC);          // streaming passes A, B, D, E
    }
    g->gridA = g->gridE = g->gridS;
    return launch ? check_launch(*g) : 0;
}

// the regions of a geometry's workspace (WsOff, eegnet_common.h); returns its size in bytes
static size_t make_layout(const Geo& g, WsOff& L) {
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = rupz(o + bytes, 256); return r; };
    // ticket words first: zero when the workspace is allocated (ops.new_workspace), re-armed by each pass's
    // reduction when it ends and, for the later passes of a call, cleared again by pass A
    L.cnt = take(CNT_BYTES);
    L.partA = take((size_t)std::max(g.gridS, g.gridA) * g.nA * 4);
    L.partB = take((size_t)std::max(std::max(g.gridS, g.grid), g.gridW2) * g.nB * 4);
    L.partC = take((size_t)std::max(g.grid, g.gridW2) * g.nC * 4);
    L.partD = take((size_t)std::max(g.grid, g.gridS) * g.nD * 4);   // (k_pass_dr: gridS; k_wpass_d: grid)
    L.partE = take((size_t)std::max(g.gridS, g.gridE) * g.nE * 4);
    const int nmax = std::max(std::max(std::max(g.nA, g.nB), std::max(g.nC, g.nD)), g.nE);
    L.sums = take((size_t)nmax * 8 * NGRPMAX);
    L.stats = take((size_t)(g.F1 * g.K1 + g.K1) * 8);   // fin1 -> fin5: G w1 per filter, window sums S1
    L.coef = take((size_t)CF_COUNT * CSTR * 4);
    const size_t per = (size_t)g.B * g.F2 * g.T1 * 4;
    L.d2 = take(per); L.E1 = take(per); L.E2 = take(per); L.dp2 = take(per);
    L.dl = take((size_t)g.B * NCLS * 4);
    // pass A's s [B][F2][T] and v [B][F2][8 ceil(T/8)] planes, read back by passes B and E
    L.s = take((size_t)g.B * g.F2 * s_pitch(g.T) * 4);
    L.v = take((size_t)g.B * g.F2 * ((g.T + 7) / 8 * 8) * 4);
    // F2 <= 16: pass B's block-2 depthwise output q and pointwise output r [B][F2][T/4], read by passes
    // C (r) and D (q, r) instead of recomputing them from d2
    L.q3 = take(per);
    L.r3 = take(per);
    return o;
}

static uint64_t mix_key(uint64_t seed, uint64_t offset) {
    uint64_t z = seed * 0xD1B54A32D192ED03ull + offset * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// dropout of one call: on when p > 0; (seed, offset) -> 64-bit key -> two per-layer 32-bit keys, threshold
static void set_key(Geo* g, uint64_t seed, uint64_t offset) {
    g->drop = g->p > 0.f ? 1 : 0;
    g->key = mix_key(seed, offset);
    g->key0 = (unsigned)g->key;
    g->key1 = (unsigned)(g->key >> 32) ^ 0x5BD1E995u;
    g->pthr = (unsigned)std::min(16777216.0, std::max(0.0, (double)g->p * 16777216.0));
}

// ---- optional per-kernel device timing (bench / roofline), off by default ----
enum KernelId { KID_A = 0, KID_B, KID_C, KID_D, KID_E, KID_ADAM, KID_INFER, KID_MEMSET, KID_INFER_BF16,
                KID_WA, KID_WB, KID_WB2, KID_WC, KID_WD, KID_WE, KID_WINFER, KID_CTAIL, KID_XSTATS, KID_INFER_DX,
                KID_COUNT };
static const char* kKernelNames[KID_COUNT] = {"k_pass_a", "k_pass_b", "k_pass_c", "k_pass_d", "k_pass_e",
                                              "k_adam", "k_infer", "memset_tickets", "k_infer_bf16",
                                              "k_wpass_a", "k_wpass_b", "k_wpass_b2", "k_wpass_c", "k_wpass_d",
                                              "k_wpass_e", "k_winfer", "k_coltail", "k_xstats", "k_infer_dx"};
#ifndef EEGNET_PROF_EVENT_FLAGS
#define EEGNET_PROF_EVENT_FLAGS hipEventDisableSystemFence
#endif
struct ProfRec { int kid; hipEvent_t a, b; };
struct ProfState { unsigned mask = 0; std::vector<ProfRec> recs; std::vector<hipEvent_t> pool; };
static thread_local ProfState g_prof;

static hipEvent_t prof_event() {
    if (!g_prof.pool.empty()) { hipEvent_t e = g_prof.pool.back(); g_prof.pool.pop_back(); return e; }
    // timing-only markers: without the system-scope release fence a default event record carries
    // (an L2 writeback + invalidate around the bracketed kernel, ~4 % of a cfg2 step with k_pass_e
    // bracketed every step: profiles/r6zb_event_fence.txt); the times are read after a full device sync
    hipEvent_t e;
    hipEventCreateWithFlags(&e, EEGNET_PROF_EVENT_FLAGS);
    return e;
}
struct ProfScope {
    int kid; hipStream_t s; hipEvent_t a = nullptr;
    ProfScope(int k, hipStream_t st) : kid(k), s(st) {
        if (k >= 0 && ((g_prof.mask >> k) & 1u)) { a = prof_event(); hipEventRecord(a, s); }
    }
    ~ProfScope() {
        if (a) { hipEvent_t b = prof_event(); hipEventRecord(b, s); g_prof.recs.push_back({kid, a, b}); }
    }
};
constexpr int KID_NONE = -1;     // a launch eegnet_profile_enable does not time

// One kernel launch: the profiled interval of `kid` brackets this launch alone; then the launch check.
// `kernel` is a pointer, so the caller picks among the instantiations of one signature (fold / single
// model, SPEC / generic, ...) in front of the call and names the arguments once; they convert to the
// kernel's parameter types here.
template <class... P, class... A>
static int launch(int kid, const char* name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes,
                  hipStream_t s, const A&... args) {
    { ProfScope prof(kid, s); hipLaunchKernelGGL(kernel, grid, block, lds_bytes, s, static_cast<P>(args)...); }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(EEGNET_ELAUNCH, "%s: %s", name, hipGetErrorString(e));
    return 0;
}

static bool g_attr_done = false;

template <int K1, int CC, int TT, int FF>
static void set_attrs_shape() {
    const int lds = LDS_MAX;
    for (const void* f : {(const void*)k_pass_a<K1, CC, TT, FF>, (const void*)k_pass_b<K1, CC, TT, FF>,
                          (const void*)k_pass_c<K1, CC, TT, FF>,
                          (const void*)k_pass_e<K1, CC, TT, FF>, (const void*)k_pass_a<K1, CC, TT, FF, true>,
                          (const void*)k_pass_b<K1, CC, TT, FF, true>, (const void*)k_pass_c<K1, CC, TT, FF, true>,
                          (const void*)k_pass_e<K1, CC, TT, FF, true>,
                          (const void*)k_pass_dr<K1, CC, TT, FF>, (const void*)k_pass_dr<K1, CC, TT, FF, false, false>,
                          (const void*)k_pass_dr<K1, CC, TT, FF, true, false>})
        hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_infer<K1, CC, TT, FF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_infer_dx<K1, CC, TT, FF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_frozen<K1, CC, TT, FF, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_frozen<K1, CC, TT, FF, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_frozen<K1, CC, TT, FF, true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    // the cut backward stages (eegnet_frozen_step_from / _folds_from), single model and fold-indexed
    for (const void* f : {(const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_AGG>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_B2>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_CLS>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, true, FZ_AGG>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, true, FZ_B2>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, true, FZ_CLS>,
                          // the windowed loader (eegnet_frozen_step_windows), every stage
                          (const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_ALL, FzWin>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_AGG, FzWin>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_B2, FzWin>,
                          (const void*)k_frozen<K1, CC, TT, FF, true, false, FZ_CLS, FzWin>})
        hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_eval_folds<K1, CC, TT, FF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_infer_win<K1, CC, TT, FF>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipFuncSetAttribute((const void*)k_infer_win<K1, CC, TT, FF, WinAtCall>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
}

template <class... S>
static void set_attrs_shapes(Shapes<S...>) { (..., set_attrs_shape<S::K1, S::CC, S::TT, S::FF>()); }

template <int K1>
static void set_attrs_wide() {
    for (const void* f : {(const void*)k_wpass_a<K1>, (const void*)k_wpass_b<K1>, (const void*)k_wpass_e<K1>,
                          (const void*)k_winfer<K1>})
        hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
}

// Every kernel a launch line gives dynamic LDS, and no other.  Eager -- the entry points call it before
// their first launch, never from inside one: fold epochs are captured into graphs.
static void ensure_attrs() {
    if (g_attr_done) return;
    set_attrs_wide<32>();
    set_attrs_wide<64>();
    for (const void* f : {(const void*)k_wpass_a<32, true>, (const void*)k_wpass_b<32, true>, (const void*)k_wpass_e<32, true>,
                          (const void*)k_winfer<32, true>, (const void*)k_wpass_b2<NTB2, true>,
                          (const void*)k_wpass_c<NTB2, true>, (const void*)k_wpass_d<NTB2, true>,
                          (const void*)k_coltail<3, true>, (const void*)k_coltail<4, true>, (const void*)k_coltail<5, true>})
        hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    for (const void* f : {(const void*)k_wpass_b2<NTB2>, (const void*)k_wpass_c<NTB2>, (const void*)k_wpass_d<NTB2>,
                          (const void*)k_coltail<3>, (const void*)k_coltail<4>, (const void*)k_coltail<5>,
                          (const void*)k_fin})
        hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    for (const void* f : {(const void*)k_infer_bf16<0>, (const void*)k_infer_bf16<1>, (const void*)k_infer_bf16<2>,
                          (const void*)k_infer_bf16<4>, (const void*)k_infer_bf16<8>, (const void*)k_infer_bf16<16>,
                          (const void*)k_infer_bf16_cfg5})
        hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    set_attrs_shape<32, 0, 0, 0>();
    set_attrs_shape<64, 0, 0, 0>();
    hipFuncSetAttribute((const void*)k_xstats<32>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    hipFuncSetAttribute((const void*)k_xstats<64>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    hipFuncSetAttribute((const void*)k_resample<float>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    hipFuncSetAttribute((const void*)k_resample<double>, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
    set_attrs_shapes(NarrowShapes{});
    g_attr_done = true;
}

// The one shape switch: f(Shape<K1, CC, TT, FF>{}) for the compile-time shape specialisations
// (NarrowShapes, eegnet_geometry.h), for any other shape the runtime-shape instantiation
// (CC = TT = FF = 0) of its K1.  The wide kernels take K1 alone.
#define SHAPE_OF(sh) decltype(sh)::K1, decltype(sh)::CC, decltype(sh)::TT, decltype(sh)::FF
template <class F>
static int dispatch_shape(const Geo& g, F&& f) {
    int r = 0;
    if (NarrowShapes::any([&](auto sh) { return has_shape(model_dims(g), sh) && (r = f(sh), true); })) return r;
    return g.K1 == 32 ? f(Shape<32, 0, 0, 0>{}) : f(Shape<64, 0, 0, 0>{});
}

// One call of the five-pass step, as its launches see it.  An entry point fills what it has; the rest
// stays null / off.  A fold-indexed launch (fc.folds, nf folds in the grid's y) has no workspace or
// pointers of its own: its kernels take every pointer and their FinArgs from the fold's record, so they
// are launched with null pointers and a zeroed FinArgs.
struct StepCall {
    char* ws;                             // the workspace (null in fold launches) and its layout
    WsOff off;
    hipStream_t s;
    const float* params = nullptr;        // written only when pass E runs Adam
    float* bn = nullptr;
    const float* x = nullptr;
    const uint8_t *m2 = nullptr, *m3 = nullptr;
    const float* dlogits = nullptr;
    const int64_t* labels = nullptr;
    float *logits = nullptr, *grads = nullptr, *loss = nullptr;
    int64_t* nbt = nullptr;
    int c_mode = 0;                       // PassCMode of pass C; without PC_BWD it writes the logits alone
    bool adam = false;                    // pass E's finalize runs Adam (else: gradients only)
    float* adam_state = nullptr;          // exp_avg, then exp_avg_sq
    int32_t* step = nullptr;
    float lr = 0.f, b1 = 0.f, b2 = 0.f, eps = 0.f;
    FoldCall fc = {};
    int nf = 1, only = -1;                // only >= 0: that pass alone (eegnet_train_stage)
    StepCall(const Geo& g, void* w, void* stream) : ws((char*)w), s((hipStream_t)stream) { make_layout(g, off); }
    // a plane or the partial rows of the workspace, as the kernels' float pointer
    float* at(unsigned long long o) const { return ws ? (float*)(ws + o) : nullptr; }
};

static FinArgs no_fin() { FinArgs f; memset(&f, 0, sizeof(f)); return f; }

// the finalize arguments of pass `tk`: what kPass (eegnet_common.h) gives the pass, from the call
static FinArgs pass_fin(const Geo& g, const StepCall& c, int tk) {
    FinArgs f = no_fin();
    if (c.fc.folds) return f;             // (fold_fin, on the device)
    const PassInfo& p = kPass[tk];
    f.part2 = (double*)(c.ws + c.off.sums);
    f.cnt = tkw((unsigned*)(c.ws + c.off.cnt), tk * NCNT);
    f.stats = (double*)(c.ws + c.off.stats);
    f.coef = c.at(c.off.coef);
    f.bn = p.bn ? c.bn : nullptr; f.nbt = p.nbt ? c.nbt : nullptr;
    f.grads = p.grads ? c.grads : nullptr; f.loss = p.loss ? c.loss : nullptr;
    f.update_running = p.update_running; f.ce = p.ce && (c.c_mode & PC_CE);
    f.tpass = tk;
    if (p.adam && c.adam) {
        f.params = const_cast<float*>(c.params);
        f.adam_m = c.adam_state; f.adam_v = c.adam_state + g.nparam; f.step = c.step;
        f.lr = c.lr; f.b1 = c.b1; f.b2 = c.b2; f.eps = c.eps;
    }
    return f;
}

// the dims the SPEC instantiations of the wide kernels are compiled for (kGeoW5, eegnet_geometry.h)
static bool spec_w5(const Geo& g) { return is_cfg5(model_dims(g)); }

// k_wpass_b keeps nothing in LDS and needs 38 VGPRs at cfg5: two 16-wave workgroups per CU (elementwise,
// so the grid does not touch the numerics)
static int grid_wpass_b(const Geo& g, bool sp) { return sp ? std::min(2 * g.gridS, g.B * g.NOC) : g.gridS; }

// F2 > 16: passes A, B (no reduction), B2 (BN3 statistics)
static int run_forward_wide(const Geo& g, const StepCall& c) {
    const WsOff& L = c.off;
    const bool sp = spec_w5(g);       // the SPEC instantiations (cfg5 shape, compile-time geometry)
    return dispatch_shape(g, [&](auto sh) {
        constexpr int K1 = decltype(sh)::K1;
        if (int r = launch(KID_WA, "k_wpass_a", sp ? k_wpass_a<K1, K1 == 32> : k_wpass_a<K1>, dim3(g.gridS),
                           dim3(NTW), g.ldsWA * 4, c.s, g, c.params, c.x, c.at(L.s), c.at(L.v), c.at(L.partA),
                           pass_fin(g, c, TK_A))) return r;
        if (int r = launch(KID_WB, "k_wpass_b", sp ? k_wpass_b<K1, K1 == 32> : k_wpass_b<K1>,
                           dim3(grid_wpass_b(g, sp)), dim3(NTW), g.ldsWB * 4, c.s, g, c.params, c.at(L.coef),
                           c.at(L.v), c.m2, c.at(L.d2), c.at(L.E1), c.at(L.E2))) return r;
        return launch(KID_WB2, "k_wpass_b2", sp ? k_wpass_b2<NTB2, true> : k_wpass_b2<NTB2>, dim3(g.gridW2),
                      dim3(NTB2), g.ldsWB2 * 4, c.s, g, c.params, c.at(L.d2), c.at(L.q3), c.at(L.r3),
                      c.at(L.partB), pass_fin(g, c, TK_B));
    });
}

// the column-parallel reduction + finalize `fin` of a split wide pass (k_coltail, eegnet_finalize.hip)
static int coltail(const Geo& g, const StepCall& c, const char* name, int fin, unsigned long long part, int nrows,
                   int ncols, const FinArgs& fa, int scr) {
    const bool sp = spec_w5(g);
    const int nb = (ncols + 63) / 64;
    const size_t lds = 8 * (size_t)std::max(2 + (NTCT / 64) * 64, tail_s_doubles(ncols) + scr);
    auto k = fin == 3 ? (sp ? k_coltail<3, true> : k_coltail<3>)
           : fin == 4 ? (sp ? k_coltail<4, true> : k_coltail<4>) : (sp ? k_coltail<5, true> : k_coltail<5>);
    return launch(KID_CTAIL, name, k, dim3(nb), dim3(NTCT), lds, c.s, g, c.params, c.at(part), nrows, ncols, fa);
}

// Pass C, the one launch line of each path.  With PC_BWD it is the backward's first pass; without
// (eegnet_forward_train) it writes the logits alone: no dl, no partial rows, no finalize.
static int run_pass_c(const Geo& g, const StepCall& c) {
    const WsOff& L = c.off;
    const bool bwd = c.c_mode & PC_BWD;
    const FinArgs fa = bwd ? pass_fin(g, c, TK_C) : no_fin();
    float *const dl = bwd ? c.at(L.dl) : nullptr, *const part = bwd ? c.at(L.partC) : nullptr;
    if (g.wide) {
        const bool sp = spec_w5(g);
        if (int r = launch(KID_WC, bwd ? "k_wpass_c(bwd)" : "k_wpass_c(fwd)", sp ? k_wpass_c<NTB2, true> : k_wpass_c<NTB2>,
                           dim3(g.gridW2), dim3(NTB2), g.ldsWC * 4, c.s, g, c.params, c.at(L.coef), c.at(L.r3), c.m3,
                           c.dlogits, c.labels, c.logits, dl, part, c.c_mode, fa)) return r;
        return bwd && g.splitC ? coltail(g, c, "k_coltail(C)", 3, L.partC, g.gridW2, g.nC, fa, 0) : 0;
    }
    return dispatch_shape(g, [&](auto sh) {
        return launch(KID_C, bwd ? "k_pass_c(bwd)" : "k_pass_c(fwd)",
                      c.fc.folds ? k_pass_c<SHAPE_OF(sh), true> : k_pass_c<SHAPE_OF(sh)>, dim3(g.grid, c.nf),
                      dim3(64 * g.nwC), g.ldsC * 4, c.s, g, c.params, c.at(L.coef), c.at(L.r3), c.m3, c.dlogits,
                      c.labels, c.logits, dl, part, c.c_mode, fa, c.fc);
    });
}

// F2 > 16: passes C, D, E, each with its k_coltail where its rows are wide
static int run_backward_wide(const Geo& g, const StepCall& c) {
    const WsOff& L = c.off;
    const float* dl = c.dlogits ? c.dlogits : c.at(L.dl);
    const FinArgs fd = pass_fin(g, c, TK_D), fe = pass_fin(g, c, TK_E);
    const bool sp = spec_w5(g);
    if (int r = run_pass_c(g, c)) return r;
    if (int r = launch(KID_WD, "k_wpass_d", sp ? k_wpass_d<NTB2, true> : k_wpass_d<NTB2>, dim3(g.grid),
                       dim3(NTB2), g.ldsWD * 4, c.s, g, c.params, c.at(L.coef), c.at(L.d2), c.at(L.E1), c.at(L.E2),
                       c.at(L.q3), c.at(L.r3), c.m2, c.m3, dl, c.at(L.dp2), c.at(L.partD), fd)) return r;
    if (g.splitD)
        if (int r = coltail(g, c, "k_coltail(D)", 4, L.partD, g.grid, g.nD, fd, 0)) return r;
    if (int r = dispatch_shape(g, [&](auto sh) {
            constexpr int K1 = decltype(sh)::K1;
            return launch(KID_WE, "k_wpass_e", sp ? k_wpass_e<K1, K1 == 32> : k_wpass_e<K1>, dim3(g.gridS), dim3(NTW),
                          g.ldsWE * 4, c.s, g, c.params, c.at(L.coef), c.x, c.at(L.s), c.at(L.v), c.at(L.dp2),
                          c.at(L.partE), fe);
        })) return r;
    // one partial row per trial range (k_wpass_e's chunk workgroups share it, disjoint columns)
    if (g.splitE)
        return coltail(g, c, "k_coltail(E)", 5, L.partE, g.gridS / g.NOC, g.nE, fe,
                       fin5_scratch_doubles(g.K1, g.F1, g.o_g2));
    return 0;
}

// passes A and B
static int run_forward(const Geo& g, const StepCall& c) {
    if (g.wide) return run_forward_wide(g, c);
    const WsOff& L = c.off;
    const bool fold = c.fc.folds;
    return dispatch_shape(g, [&](auto sh) {
        if (c.only < 0 || c.only == TK_A)
            if (int r = launch(KID_A, "k_pass_a", fold ? k_pass_a<SHAPE_OF(sh), true> : k_pass_a<SHAPE_OF(sh)>,
                               dim3(g.gridA, c.nf), dim3(NTB), g.ldsA * 4, c.s, g, c.params, c.x, c.at(L.s), c.at(L.v),
                               c.at(L.partA), pass_fin(g, c, TK_A), c.fc)) return r;
        if (c.only < 0 || c.only == TK_B)
            return launch(KID_B, "k_pass_b", fold ? k_pass_b<SHAPE_OF(sh), true> : k_pass_b<SHAPE_OF(sh)>,
                          dim3(g.gridS, c.nf), dim3(NTB), g.ldsB * 4, c.s, g, c.params, c.at(L.coef), c.at(L.v), c.m2,
                          c.at(L.d2), c.at(L.E1), c.at(L.E2), c.at(L.q3), c.at(L.r3), c.at(L.partB),
                          pass_fin(g, c, TK_B), c.fc);
        return 0;
    });
}

// passes C, D and E
static int run_backward(const Geo& g, const StepCall& c) {
    if (g.wide) return run_backward_wide(g, c);
    const WsOff& L = c.off;
    const bool fold = c.fc.folds;
    const float* dl = c.dlogits ? c.dlogits : c.at(L.dl);
    if (c.only < 0 || c.only == TK_C)
        if (int r = run_pass_c(g, c)) return r;
    return dispatch_shape(g, [&](auto sh) {
        if (c.only < 0 || c.only == TK_D) {
            // fold launches and the device generator run the instantiation without the host-mask path
            // (the profile label and the error string stay "k_pass_d": bench and tests match on them)
            auto k = fold ? k_pass_dr<SHAPE_OF(sh), true, false>
                   : (c.m2 || c.m3) ? k_pass_dr<SHAPE_OF(sh)> : k_pass_dr<SHAPE_OF(sh), false, false>;
            if (int r = launch(KID_D, "k_pass_d", k, dim3(g.gridS, c.nf), dim3(NTB), g.ldsD * 4, c.s, g, c.params,
                               c.at(L.coef), c.at(L.d2), c.at(L.E1), c.at(L.E2), c.at(L.q3), c.at(L.r3), c.m2, c.m3, dl,
                               c.at(L.dp2), c.at(L.partD), pass_fin(g, c, TK_D), c.fc)) return r;
        }
        if (c.only < 0 || c.only == TK_E)
            return launch(KID_E, "k_pass_e", fold ? k_pass_e<SHAPE_OF(sh), true> : k_pass_e<SHAPE_OF(sh)>,
                          dim3(g.gridE, c.nf), dim3(NTB), g.ldsE * 4, c.s, g, c.params, c.at(L.coef), c.x, c.at(L.s),
                          c.at(L.v), c.at(L.dp2), c.at(L.partE), pass_fin(g, c, TK_E), c.fc);
        return 0;
    });
}

// geometry of the bf16 eval kernel (eegnet_infer_bf16.hip)
static float* g_bf16_dbg = nullptr;     // eegnet_debug_bf16 (debug builds only)

static int make_geo_bf16(const eegnet_dims* d, GeoI* g) {
    if (int r = check_dims(d)) return r;
    *g = geo_shape_bf16(model_dims(*d));
    g->B = d->B;
    g->eps = d->bn_eps;
    g->dbg = g_bf16_dbg;
    if (g->PFU > 16) return fail(EEGNET_EINVAL, "bf16 eval: C*T too large for one trial in registers");
    if (g->lds > LDS_MAX)
        return fail(EEGNET_EINVAL, "bf16 eval: dims need %d B of LDS (> %d): C=%d T=%d F2=%d", g->lds, LDS_MAX,
                    g->C, g->T, g->F2);
    return 0;
}

// The train step of the F2 > 16 path with 64 temporal taps (k_wpass_a<64> / k_wpass_e<64>) is refused:
// at EEGNet-8,4 on 5 x 72 (B = 513) it ended in a GPU memory fault whose cause is not known, and no
// test has seen it produce a result.  The eval forward of these dims (k_winfer<64>) is tested and stays.
static int check_wide_train(const Geo& g, const char* what) {
    if (g.wide && g.K1 == 64)
        return fail(EEGNET_EINVAL, "%s: training with F1*D = %d > 16 and K1 = 64 is not supported "
                    "(K1 = 32, or F1*D <= 16; the eval forward takes these dims)", what, g.F2);
    return 0;
}

static int check_ptrs(const void* a, const char* na, const void* b = (const void*)1, const char* nb = "") {
    if (!a) return fail(EEGNET_EINVAL, "%s is NULL", na);
    if (!b) return fail(EEGNET_EINVAL, "%s is NULL", nb);
    return 0;
}

// flags outside `known` are refused, in the entry point's words (`fmt` takes the unknown bits as %x)
static int check_flags(int flags, int known, const char* fmt) {
    return (flags & ~known) ? fail(EEGNET_EINVAL, fmt, flags & ~known) : 0;
}

// geometry of an entry point the F2 > 16 path does not implement: wide dims are refused before the wide
// kernels' launch limits are looked at
static int make_geo_narrow(const eegnet_dims* d, Geo* g, const char* what, bool launch = true) {
    if (int r = make_geo(d, g, false)) return r;
    if (g->wide) return fail(EEGNET_EINVAL, "%s: F1*D = %d > 16 is not supported", what, g->F2);
    return launch ? make_geo(d, g) : 0;
}

// the flags, dropout keys and (EEGNET_KEY_FROM_STEP) device-side key of a train call
static int train_flags(Geo* g, int flags, uint64_t seed, uint64_t offset, const int32_t* step) {
    g->noclamp = (flags & EEGNET_NO_CLAMP) ? 1 : 0;
    set_key(g, seed, offset);
    if (flags & EEGNET_KEY_FROM_STEP) {
        if (!step) return fail(EEGNET_EINVAL, "EEGNET_KEY_FROM_STEP needs the device step counter");
        g->keystep = step; g->kseed = seed; g->koff = offset;
    }
    return 0;
}

extern "C" {

int eegnet_param_count(const eegnet_dims* dims, int64_t* out) {
    Geo g;
    if (int r = make_geo(dims, &g, false)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    *out = g.nparam;
    return 0;
}

int eegnet_x_pitch(const eegnet_dims* dims) {
    if (!dims) return fail(EEGNET_EINVAL, "dims is NULL");
    return x_pitch_shape(model_dims(*dims)) ? (dims->T + 3) & ~3 : dims->T;
}

int eegnet_wide_spec(const eegnet_dims* dims) {
    if (int r = check_dims(dims)) return r;
    return is_cfg5(model_dims(*dims));
}

int eegnet_workspace_bytes(const eegnet_dims* dims, size_t* out) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    WsOff L;
    *out = make_layout(g, L);
    return 0;
}

int eegnet_forward_train(const eegnet_dims* dims, const float* params, float* bn_buffers,
                         const float* x, const uint8_t* mask2, const uint8_t* mask3,
                         uint64_t seed, uint64_t offset, float* logits, void* ws, void* stream,
                         int64_t* num_batches_tracked) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (int r = check_wide_train(g, "eegnet_forward_train")) return r;
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", logits, "logits")) return r;
    if (int r = check_ptrs(ws, "ws")) return r;
    set_key(&g, seed, offset);
    ensure_attrs();
    StepCall c(g, ws, stream);
    c.params = params; c.bn = bn_buffers; c.x = x; c.m2 = mask2; c.m3 = mask3;
    c.logits = logits; c.nbt = num_batches_tracked;
    c.c_mode = PC_LOGITS;                 // pass C for the logits alone: no labels, no dlogits
    if (int r = run_forward(g, c)) return r;
    return run_pass_c(g, c);
}

int eegnet_backward(const eegnet_dims* dims, const float* params, const float* x,
                    const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                    const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads, float* loss,
                    void* ws, void* stream, int flags) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (int r = check_wide_train(g, "eegnet_backward")) return r;
    g.noclamp = (flags & EEGNET_NO_CLAMP) ? 1 : 0;
    if (int r = check_ptrs(params, "params", x, "x")) return r;
    if (int r = check_ptrs(grads, "grads", ws, "ws")) return r;
    if (!dlogits && !labels) return fail(EEGNET_EINVAL, "need dlogits or labels");
    set_key(&g, seed, offset);
    ensure_attrs();
    StepCall c(g, ws, stream);
    c.params = params; c.x = x; c.m2 = mask2; c.m3 = mask3;
    c.dlogits = dlogits; c.labels = labels; c.grads = grads; c.loss = loss;
    c.c_mode = PC_BWD | (dlogits ? 0 : PC_CE);
    return run_backward(g, c);
}

int eegnet_forward_eval(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                        const float* x, float* logits, void* stream) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (g.XP != g.T) return fail(EEGNET_EINVAL, "the eval forward takes x as [B][C][T] (x_pitch 0 or T)");
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", logits, "logits")) return r;
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    return dispatch_shape(g, [&](auto sh) {
        constexpr int K1 = decltype(sh)::K1;
        if (g.wide)
            return launch(KID_WINFER, "k_winfer", spec_w5(g) ? k_winfer<K1, K1 == 32> : k_winfer<K1>, dim3(g.grid),
                          dim3(NTW), g.ldsWI * 4, s, g, params, bn_buffers, x, logits);
        return launch(KID_INFER, "k_infer", k_infer<SHAPE_OF(sh)>, dim3(g.grid), dim3(NTH), g.ldsI * 4, s, g, params,
                      bn_buffers, x, logits);
    });
}

// the PLANE plan of eegnet_trial.hip has to fit the LDS (k_infer_dx, k_frozen)
static int check_lds_x(const Geo& g, const char* what) {
    if (g.ldsX * 4 > LDS_MAX) return fail(EEGNET_EINVAL, "%s: dims need %d B of LDS (> %d)", what, g.ldsX * 4, LDS_MAX);
    return 0;
}

int eegnet_input_grad_eval(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                           const float* x, int seed_kind, const float* dlogits, const int64_t* targets,
                           float* dx, float* logits, void* stream) {
    Geo g;
    if (int r = make_geo_narrow(dims, &g, "input gradients")) return r;
    if (g.XP != g.T) return fail(EEGNET_EINVAL, "input gradients take x as [B][C][T] (x_pitch 0 or T)");
    if (seed_kind < EEGNET_SEED_DLOGITS || seed_kind > EEGNET_SEED_CE)
        return fail(EEGNET_EINVAL, "seed_kind must be 0 (dlogits), 1 (logit) or 2 (cross-entropy) (got %d)", seed_kind);
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", dx, "dx")) return r;
    if (seed_kind == EEGNET_SEED_DLOGITS && !dlogits) return fail(EEGNET_EINVAL, "EEGNET_SEED_DLOGITS needs dlogits");
    if (seed_kind == EEGNET_SEED_CE && !targets) return fail(EEGNET_EINVAL, "EEGNET_SEED_CE needs targets");
    if (int r = check_lds_x(g, "input gradients")) return r;
    if ((g.T & 3) == 0 && ((uintptr_t)x & 15)) return fail(EEGNET_EINVAL, "input gradients: x must be 16-byte aligned");
    // dx rows go out in 16-byte stores only when every row of it starts 16-byte aligned
    const int vec = (g.T & 3) == 0 && ((uintptr_t)dx & 15) == 0;
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    return dispatch_shape(g, [&](auto sh) {
        return launch(KID_INFER_DX, "k_infer_dx", k_infer_dx<SHAPE_OF(sh)>, dim3(g.grid), dim3(NTH), g.ldsX * 4, s, g,
                      params, bn_buffers, x, seed_kind, dlogits, targets, dx, logits, vec);
    });
}

int eegnet_forward_eval_bf16(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                             const uint16_t* x, float* logits, void* stream) {
    GeoI g;
    if (int r = make_geo_bf16(dims, &g)) return r;
    if (dims->x_pitch && dims->x_pitch != dims->T)
        return fail(EEGNET_EINVAL, "the eval forward takes x as [B][C][T] (x_pitch 0 or T)");
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", logits, "logits")) return r;
    if (g.PFU > 0 && ((uintptr_t)x & 15))
        return fail(EEGNET_EINVAL, "bf16 eval: x must be 16-byte aligned");
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    // cfg5: the time-chunked kernel, two workgroups per CU (eegnet_infer_bf16c.hip)
    if (is_cfg5(model_dims(g)))
        return launch(KID_INFER_BF16, "k_infer_bf16(cfg5)", k_infer_bf16_cfg5, dim3(std::min(g.B, 2 * device_cus())),
                      dim3(c5::NT), c5::LDS, s, g, params, bn_buffers, x, logits);
    // the whole-trial kernel, by the prefetch registers per thread
    auto k = g.PFU == 0 ? k_infer_bf16<0> : g.PFU == 1 ? k_infer_bf16<1> : g.PFU == 2 ? k_infer_bf16<2>
           : g.PFU == 4 ? k_infer_bf16<4> : g.PFU == 8 ? k_infer_bf16<8> : k_infer_bf16<16>;
    return launch(KID_INFER_BF16, "k_infer_bf16", k, dim3(std::min(g.B, device_cus())), dim3(NTI), g.lds, s, g, params,
                  bn_buffers, x, logits);
}

int eegnet_adam_step(int64_t n, float* params, const float* grads, float* exp_avg,
                     float* exp_avg_sq, int32_t* step, float lr, float beta1, float beta2,
                     float eps, void* stream) {
    if (n <= 0) return fail(EEGNET_EINVAL, "n must be > 0");
    if (!params || !grads || !exp_avg || !exp_avg_sq || !step) return fail(EEGNET_EINVAL, "null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (int r = launch(KID_ADAM, "k_adam", k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, params, grads,
                       exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps)) return r;
    return launch(KID_NONE, "k_step_inc", k_step_inc, dim3(1), dim3(64), 0, s, step);
}

int eegnet_train_step(const eegnet_dims* dims, float* params, float* bn_buffers, const float* x,
                      const int64_t* labels, uint64_t seed, uint64_t offset, float* grads,
                      float* adam_state, int32_t* step, float lr, float beta1, float beta2,
                      float eps, float* loss, float* logits, void* ws, void* stream, int flags,
                      int64_t* num_batches_tracked) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (int r = check_wide_train(g, "eegnet_train_step")) return r;
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", labels, "labels")) return r;
    if (int r = check_ptrs(grads, "grads", ws, "ws")) return r;
    if (adam_state && !step) return fail(EEGNET_EINVAL, "step is NULL");
    if (int r = check_flags(flags, EEGNET_NO_CLAMP | EEGNET_KEY_FROM_STEP,
                            "unknown flags 0x%x (bit 4, round 5's opt-in persistent step, is retired)")) return r;
    if (int r = train_flags(&g, flags, seed, offset, step)) return r;
    ensure_attrs();
    StepCall c(g, ws, stream);
    c.params = params; c.bn = bn_buffers; c.x = x; c.labels = labels;
    c.logits = logits; c.grads = grads; c.loss = loss; c.nbt = num_batches_tracked;
    c.c_mode = PC_BWD | PC_CE | (logits ? PC_LOGITS : 0);
    // Adam runs in pass E's finalize; adam_state == NULL: gradients only (data-parallel: all-reduce,
    // clamp, then eegnet_adam_step)
    c.adam = adam_state != nullptr;
    c.adam_state = adam_state; c.step = step; c.lr = lr; c.b1 = beta1; c.b2 = beta2; c.eps = eps;
    if (int r = run_forward(g, c)) return r;
    return run_backward(g, c);
}

// One stage of a data-parallel train step with synchronised BatchNorm (distributed.py
// DataParallelTrainer(sync_bn=True)): stage 2k launches pass k (A..E) with its finalize deferred --
// the reduction's winner leaves the pass's fp64 sums at eegnet_stage_sums' place in the workspace for
// the host to all-reduce over the ranks --, stage 2k + 1 runs pass k's finalize (k_fin) on the reduced
// sums.  norm_batch: the global batch (BN statistics, the CE mean), so every finalize sees global-batch
// sums and the gradients, running statistics, clamps and Adam come out identical on every rank.
int eegnet_train_stage(const eegnet_dims* dims, int stage, int64_t norm_batch, float* params, float* bn_buffers,
                       const float* x, const int64_t* labels, uint64_t seed, uint64_t offset, float* grads,
                       float* adam_state, int32_t* step, float lr, float beta1, float beta2, float eps,
                       float* loss, void* ws, void* stream, int flags, int64_t* num_batches_tracked) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (g.wide) return fail(EEGNET_EINVAL, "eegnet_train_stage: F1*D = %d > 16 is not supported", g.F2);
    if (stage < 0 || stage >= 2 * TK_COUNT) return fail(EEGNET_EINVAL, "stage must be in [0, %d) (got %d)", 2 * TK_COUNT, stage);
    if (norm_batch < g.B || norm_batch > (1LL << 30))
        return fail(EEGNET_EINVAL, "norm_batch must be in [B, 2^30] (got %lld)", (long long)norm_batch);
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", labels, "labels")) return r;
    if (int r = check_ptrs(grads, "grads", ws, "ws")) return r;
    if (adam_state && !step) return fail(EEGNET_EINVAL, "step is NULL");
    g.Bn = (int)norm_batch;
    if (int r = train_flags(&g, flags, seed, offset, step)) return r;
    ensure_attrs();
    const int pass = stage >> 1;
    const bool fin = stage & 1;
    g.defer = 1;                  // (k_fin: fin5 runs the whole Adam update, adam_early is off)
    StepCall c(g, ws, stream);
    c.params = params; c.bn = bn_buffers; c.x = x; c.labels = labels;
    c.grads = grads; c.loss = loss; c.nbt = num_batches_tracked;
    c.c_mode = PC_BWD | PC_CE;
    c.adam = fin && adam_state;   // Adam is the finalize stage's; the pass is launched for its gradients only
    c.adam_state = adam_state; c.step = step; c.lr = lr; c.b1 = beta1; c.b2 = beta2; c.eps = eps;
    c.only = pass;
    if (!fin) return pass <= TK_B ? run_forward(g, c) : run_backward(g, c);
    return launch(KID_NONE, "k_fin", k_fin, dim3(1), dim3(NTB), (size_t)(g.*kPass[pass].lds) * 4, c.s, g, params,
                  pass_fin(g, c, pass), pass, g.*kPass[pass].ncols);
}

// where stage 2k leaves pass k's sums in a workspace: byte offset and count of fp64 values
int eegnet_stage_sums(const eegnet_dims* dims, int pass, size_t* offset_bytes, int* count) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (pass < 0 || pass >= TK_COUNT) return fail(EEGNET_EINVAL, "pass must be in [0, %d) (got %d)", TK_COUNT, pass);
    if (!offset_bytes || !count) return fail(EEGNET_EINVAL, "null output pointer");
    WsOff L;
    make_layout(g, L);
    *offset_bytes = L.sums;
    *count = g.*kPass[pass].ncols;
    return 0;
}

}  // extern "C"

// ---- frozen-BatchNorm fine-tuning (eegnet_frozen.hip) ----
// the checks eegnet_forward_frozen and eegnet_frozen_step share; none needs a GPU
static int frozen_geo(const eegnet_dims* dims, Geo* g) {
    if (int r = make_geo_narrow(dims, g, "frozen BatchNorm")) return r;
    if (g->XP != g->T) return fail(EEGNET_EINVAL, "frozen BatchNorm takes x as [B][C][T] (x_pitch 0 or T)");
    if (int r = check_lds_x(*g, "frozen BatchNorm")) return r;
    if (g->NF > NTH) return fail(EEGNET_EINVAL, "frozen BatchNorm: F2*(T/32) = %d > %d", g->NF, NTH);
    return 0;
}

static size_t frozen_ws_bytes(const Geo& g) { return rupz((size_t)g.grid * fz_cols(g).n * 4, 256); }

// the backward instantiation of a shape for train_from (EEGNET_TRAIN_*, validated by frozen_offset)
// (Src: the loader policy, FzWin for the windows of a table)
template <int K1, int CC, int TT, int FF, bool FOLD, class Src = FzFold<FOLD>>
static auto frozen_bwd_kernel(int train_from) {
    switch (train_from) {
        case EEGNET_TRAIN_FROM_AGGREGATION: return k_frozen<K1, CC, TT, FF, true, FOLD, FZ_AGG, Src>;
        case EEGNET_TRAIN_FROM_BLOCK2: return k_frozen<K1, CC, TT, FF, true, FOLD, FZ_B2, Src>;
        case EEGNET_TRAIN_FROM_CLASSIFIER: return k_frozen<K1, CC, TT, FF, true, FOLD, FZ_CLS, Src>;
        default: return k_frozen<K1, CC, TT, FF, true, FOLD, FZ_ALL, Src>;
    }
}

static int frozen_launch(const char* name, const Geo& g, bool bwd, int train_from, const float* params,
                         const float* bn, const float* x, const float* dlogits, const int64_t* labels,
                         const uint8_t* m2, const uint8_t* m3, float* logits, float* part, hipStream_t s,
                         const FzWin* win = nullptr) {
    return dispatch_shape(g, [&](auto sh) {
        if (win)                                      // x and the labels through the table (x is unused)
            return launch(KID_NONE, name, frozen_bwd_kernel<SHAPE_OF(sh), false, FzWin>(train_from), dim3(g.grid),
                          dim3(NTH), g.ldsX * 4, s, g, params, bn, x, dlogits, labels, m2, m3, logits, part, *win);
        return launch(KID_NONE, name,
                      bwd ? frozen_bwd_kernel<SHAPE_OF(sh), false>(train_from) : k_frozen<SHAPE_OF(sh), false>,
                      dim3(g.grid), dim3(NTH), g.ldsX * 4, s, g, params, bn, x, dlogits, labels, m2, m3, logits, part,
                      FzFold<false>{});
    });
}

// first element of the trainable suffix of the flat parameters for train_from: the flat buffer is in
// network order, so freezing every module before one freezes a prefix of it
static int frozen_offset(const Geo& g, int train_from, int* off) {
    switch (train_from) {
        case EEGNET_TRAIN_ALL: *off = 0; return 0;
        case EEGNET_TRAIN_FROM_AGGREGATION: *off = g.o_g2; return 0;
        case EEGNET_TRAIN_FROM_BLOCK2: *off = g.o_w2; return 0;
        case EEGNET_TRAIN_FROM_CLASSIFIER: *off = g.o_Wfc; return 0;
    }
    return fail(EEGNET_EINVAL, "train_from must be EEGNET_TRAIN_ALL (0), EEGNET_TRAIN_FROM_AGGREGATION (1), "
                "EEGNET_TRAIN_FROM_BLOCK2 (2) or EEGNET_TRAIN_FROM_CLASSIFIER (3) (got %d)", train_from);
}

// The arguments every fold-indexed step takes, checked, as the kernels' FoldCall; `off`, the workspace
// layout of the five-pass step, stays zero for the caller to assign.
static int fold_call(FoldCall* fc, int nfolds, const eegnet_fold* folds, int64_t row0, int64_t slot, uint64_t offset,
                     float lr, float beta1, float beta2, float eps) {
    if (nfolds < 1 || nfolds > 65535) return fail(EEGNET_EINVAL, "nfolds must be in [1, 65535] (got %d)", nfolds);
    if (!folds) return fail(EEGNET_EINVAL, "folds is NULL");
    if (row0 < 0 || slot < 0) return fail(EEGNET_EINVAL, "row0 / slot must be >= 0");
    memset(fc, 0, sizeof(*fc));
    fc->folds = folds;
    fc->row0 = row0; fc->slot = slot; fc->koff = offset;
    fc->lr = lr; fc->b1 = beta1; fc->b2 = beta2; fc->eps = eps;
    return 0;
}

// workgroups of k_frozen_reduce: FR_OUT outputs each over the gradients from `off` on and the loss
static unsigned frozen_reduce_grid(const Geo& g, int off = 0) {
    return (unsigned)((g.nparam - off + 1 + FR_OUT - 1) / FR_OUT);
}

extern "C" {

int eegnet_frozen_workspace_bytes(const eegnet_dims* dims, size_t* out) {
    Geo g;
    if (int r = frozen_geo(dims, &g)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    *out = frozen_ws_bytes(g);
    return 0;
}

int eegnet_forward_frozen(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                          const float* x, const uint8_t* mask2, const uint8_t* mask3, uint64_t seed,
                          uint64_t offset, float* logits, void* stream) {
    Geo g;
    if (int r = frozen_geo(dims, &g)) return r;
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", logits, "logits")) return r;
    if ((g.T & 3) == 0 && ((uintptr_t)x & 15)) return fail(EEGNET_EINVAL, "frozen BatchNorm: x must be 16-byte aligned");
    set_key(&g, seed, offset);
    ensure_attrs();
    return frozen_launch("k_frozen(fwd)", g, false, EEGNET_TRAIN_ALL, params, bn_buffers, x, nullptr, nullptr, mask2,
                         mask3, logits, nullptr, (hipStream_t)stream);
}

// eegnet_frozen_step_from behind its checks, for x as [B][C][T] or (win) the windows of a table: k_frozen, the
// reduction of its partial rows and, with adam_state, Adam over the trainable suffix
static int frozen_step_run(Geo& g, int off, int train_from, float* params, const float* bn_buffers, const float* x,
                           const FzWin* win, const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                           const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads, float* adam_state,
                           int32_t* step, float lr, float beta1, float beta2, float eps, float* loss, float* logits,
                           void* ws, void* stream, int flags) {
    if (int r = train_flags(&g, flags, seed, offset, step)) return r;
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    float* part = (float*)ws;
    if (int r = frozen_launch(win ? "k_frozen(windows)" : "k_frozen", g, true, train_from, params, bn_buffers, x, dlogits,
                              labels, mask2, mask3, logits, part, s, win))
        return r;
    if (int r = launch(KID_NONE, "k_frozen_reduce", k_frozen_reduce<false>, dim3(frozen_reduce_grid(g, off)),
                       dim3(NTFR), 0, s, g, params, bn_buffers, part, g.grid, grads, loss, off, FzFold<false>{})) return r;
    if (!adam_state) return 0;
    // the Adam kernel of eegnet_adam_step behind the reduction, over the trainable suffix; it advances the
    // step counter last, after k_frozen has read it for the dropout key (EEGNET_KEY_FROM_STEP)
    return eegnet_adam_step(g.nparam - off, params + off, grads + off, adam_state + off, adam_state + g.nparam + off,
                            step, lr, beta1, beta2, eps, stream);
}

int eegnet_frozen_step_from(const eegnet_dims* dims, float* params, const float* bn_buffers, const float* x,
                            const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                            const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads,
                            float* adam_state, int32_t* step, float lr, float beta1, float beta2, float eps,
                            float* loss, float* logits, void* ws, void* stream, int flags, int train_from) {
    Geo g;
    if (int r = frozen_geo(dims, &g)) return r;
    int off;
    if (int r = frozen_offset(g, train_from, &off)) return r;
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(x, "x", grads, "grads")) return r;
    if (int r = check_ptrs(ws, "ws")) return r;
    if (!dlogits && !labels) return fail(EEGNET_EINVAL, "frozen step: need dlogits or labels");
    if (dlogits && labels) return fail(EEGNET_EINVAL, "frozen step: dlogits and labels are exclusive");
    if (adam_state && !step) return fail(EEGNET_EINVAL, "step is NULL");
    if (int r = check_flags(flags, EEGNET_NO_CLAMP | EEGNET_KEY_FROM_STEP, "frozen step: unknown flags 0x%x")) return r;
    if ((g.T & 3) == 0 && ((uintptr_t)x & 15)) return fail(EEGNET_EINVAL, "frozen BatchNorm: x must be 16-byte aligned");
    return frozen_step_run(g, off, train_from, params, bn_buffers, x, nullptr, dlogits, labels, mask2, mask3, seed, offset,
                           grads, adam_state, step, lr, beta1, beta2, eps, loss, logits, ws, stream, flags);
}

// The frozen step on the windows a table places in continuous recordings (FzWin, eegnet_frozen.hip): the
// checks of eegnet_frozen_step_from and of eegnet_forward_eval_windows_at, none of which needs a GPU.
int eegnet_frozen_step_windows(const eegnet_dims* dims, float* params, const float* bn_buffers, const float* rec,
                               int64_t n_rec, int64_t n_samples, int64_t pitch, const int64_t* starts,
                               const int32_t* rec_index, const int64_t* labels, int64_t n_table, const int64_t* sel,
                               const float* dlogits, const uint8_t* mask2, const uint8_t* mask3, uint64_t seed,
                               uint64_t offset, float* grads, float* adam_state, int32_t* step, float lr, float beta1,
                               float beta2, float eps, float* loss, float* logits, void* ws, void* stream, int flags,
                               int train_from) {
    Geo g;
    if (int r = frozen_geo(dims, &g)) return r;
    int off;
    if (int r = frozen_offset(g, train_from, &off)) return r;
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(rec, "rec", grads, "grads")) return r;
    if (int r = check_ptrs(starts, "starts", ws, "ws")) return r;
    if (!dlogits && !labels) return fail(EEGNET_EINVAL, "frozen step on windows: need dlogits or labels");
    if (dlogits && labels) return fail(EEGNET_EINVAL, "frozen step on windows: dlogits and labels are exclusive");
    if (adam_state && !step) return fail(EEGNET_EINVAL, "step is NULL");
    if (int r = check_flags(flags, EEGNET_NO_CLAMP | EEGNET_KEY_FROM_STEP, "frozen step on windows: unknown flags 0x%x"))
        return r;
    if (n_rec < 1 || n_rec > 2147483647)
        return fail(EEGNET_EINVAL, "frozen step on windows: n_rec must be in [1, 2^31) (got %lld)", (long long)n_rec);
    if (n_samples < g.T)
        return fail(EEGNET_EINVAL, "frozen step on windows: n_samples = %lld is shorter than one window (T = %d)",
                    (long long)n_samples, g.T);
    if (pitch < n_samples)
        return fail(EEGNET_EINVAL, "frozen step on windows: pitch = %lld is below n_samples = %lld", (long long)pitch,
                    (long long)n_samples);
    if (((uintptr_t)rec & 3) || ((uintptr_t)starts & 7) || ((uintptr_t)rec_index & 3) || ((uintptr_t)labels & 7) ||
        ((uintptr_t)sel & 7))
        return fail(EEGNET_EINVAL, "frozen step on windows: rec, starts, rec_index, labels and sel must be aligned to "
                    "their element size");
    if (n_table < 1 || n_table > 2147483647)
        return fail(EEGNET_EINVAL, "frozen step on windows: n_table must be in [1, 2^31) (got %lld)", (long long)n_table);
    if (!sel && g.B > n_table)
        return fail(EEGNET_EINVAL, "frozen step on windows: B = %d windows exceed the table's %lld entries (no sel)", g.B,
                    (long long)n_table);
    FzWin fw;
    fw.ac.rec = rec;
    fw.ac.pitch = pitch;
    fw.ac.hop = 0;
    fw.ac.W = 0;
    fw.ac.total = (int)n_table;
    fw.ac.vec = 0;
    fw.ac.starts = (const long long*)starts;
    fw.ac.rec_index = rec_index;
    fw.ac.last = n_samples - g.T;
    fw.ac.n_rec = (int)n_rec;
    fw.sel = (const long long*)sel;
    return frozen_step_run(g, off, train_from, params, bn_buffers, nullptr, &fw, dlogits, labels, mask2, mask3, seed,
                           offset, grads, adam_state, step, lr, beta1, beta2, eps, loss, logits, ws, stream, flags);
}

int eegnet_frozen_step(const eegnet_dims* dims, float* params, const float* bn_buffers, const float* x,
                       const float* dlogits, const int64_t* labels, const uint8_t* mask2,
                       const uint8_t* mask3, uint64_t seed, uint64_t offset, float* grads,
                       float* adam_state, int32_t* step, float lr, float beta1, float beta2, float eps,
                       float* loss, float* logits, void* ws, void* stream, int flags) {
    return eegnet_frozen_step_from(dims, params, bn_buffers, x, dlogits, labels, mask2, mask3, seed, offset, grads,
                                   adam_state, step, lr, beta1, beta2, eps, loss, logits, ws, stream, flags,
                                   EEGNET_TRAIN_ALL);
}

int eegnet_trainable_offset(const eegnet_dims* dims, int train_from, int64_t* out) {
    Geo g;
    if (int r = frozen_geo(dims, &g)) return r;
    int off;
    if (int r = frozen_offset(g, train_from, &off)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    *out = off;
    return 0;
}

// One frozen-BatchNorm iteration of nfolds models in four launches, whatever nfolds: k_frozen and
// k_frozen_reduce with the fold in the grid's y, then Adam and the step counters.  The per-fold grid is
// eegnet_frozen_step's for the same dims (g.grid, a function of B alone), so a fold's partial rows -- and
// with them every bit of its result -- are those of that call on the fold alone.
int eegnet_frozen_step_folds_from(const eegnet_dims* dims, int nfolds, const eegnet_fold* folds, int64_t row0,
                                  int64_t slot, uint64_t offset, float lr, float beta1, float beta2, float eps,
                                  int flags, void* stream, int train_from) {
    Geo g;
    if (int r = frozen_geo(dims, &g)) return r;
    int off;
    if (int r = frozen_offset(g, train_from, &off)) return r;
    FoldCall fc;
    if (int r = fold_call(&fc, nfolds, folds, row0, slot, offset, lr, beta1, beta2, eps)) return r;
    if (int r = check_flags(flags, EEGNET_NO_CLAMP, "frozen fold step: unknown flags 0x%x (the dropout keys always "
                            "follow the folds' device steps)")) return r;
    g.noclamp = (flags & EEGNET_NO_CLAMP) ? 1 : 0;
    set_key(&g, 0, offset);                           // the keep threshold (keys come per fold)
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    const unsigned nf = (unsigned)nfolds;
    const FzFold<true> fold{fc};
    if (int r = dispatch_shape(g, [&](auto sh) {
            return launch(KID_NONE, "k_frozen(folds)", frozen_bwd_kernel<SHAPE_OF(sh), true>(train_from), dim3(g.grid, nf),
                          dim3(NTH), g.ldsX * 4, s, g, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, fold);
        })) return r;
    if (int r = launch(KID_NONE, "k_frozen_reduce(folds)", k_frozen_reduce<true>, dim3(frozen_reduce_grid(g, off), nf),
                       dim3(NTFR), 0, s, g, nullptr, nullptr, nullptr, g.grid, nullptr, nullptr, off, fold)) return r;
    // every reader of the step counters -- the dropout keys above, Adam's bias correction -- is in an
    // earlier launch than their increment
    if (int r = launch(KID_NONE, "k_adam_folds", k_adam_folds, dim3((unsigned)((g.nparam - off + 255) / 256), nf),
                       dim3(256), 0, s, (int64_t)g.nparam, (int64_t)off, fc)) return r;
    return launch(KID_NONE, "k_step_inc_folds", k_step_inc_folds, dim3((nf + 255) / 256), dim3(256), 0, s, fc, nfolds);
}

int eegnet_frozen_step_folds(const eegnet_dims* dims, int nfolds, const eegnet_fold* folds, int64_t row0,
                             int64_t slot, uint64_t offset, float lr, float beta1, float beta2, float eps,
                             int flags, void* stream) {
    return eegnet_frozen_step_folds_from(dims, nfolds, folds, row0, slot, offset, lr, beta1, beta2, eps, flags, stream,
                                         EEGNET_TRAIN_ALL);
}

}  // extern "C"

// trials per workgroup of the fold-indexed launches: the streaming-grid passes A / B / D (k_pass_dr) /
// E, pass C; a -DEEGNET_FOLD_TPW_S / _A / _E / _C build overrides them (sweeps, tools/r6_tpw.sh).  Chosen over 12, 23, 45 and 90 resident folds of batch 64
// (22 x 257): 4 trials per streaming workgroup; pass C one trial per wave of its 16 (round 6:
// 16 instead of 8 left no wave idle, +3 % at 12 folds and +5-6 % at 45 / 90).
#ifndef EEGNET_FOLD_TPW_S
#define EEGNET_FOLD_TPW_S 4
#endif
#ifndef EEGNET_FOLD_TPW_A
#define EEGNET_FOLD_TPW_A EEGNET_FOLD_TPW_S
#endif
#ifndef EEGNET_FOLD_TPW_E
#define EEGNET_FOLD_TPW_E EEGNET_FOLD_TPW_S
#endif
#ifndef EEGNET_FOLD_TPW_C
#define EEGNET_FOLD_TPW_C 16
#endif

// The per-fold grids of a fold-indexed launch.  The folds share the chip: each workgroup runs several
// trials of its fold (its prologue and the reduction tail are per workgroup).  The per-fold grid is a
// function of B alone -- never of nfolds -- so a fold's trial -> workgroup split, and with it every
// partial sum and every bit of its result, does not depend on how many folds share the launch
// (fold-batch width, sharding over ranks).  Capped at the non-fold grids the workspace's partial rows
// are sized for.
static void fold_grids(Geo* g) {
    const auto split = [&](int cap, int tpw) { return std::max(1, std::min(cap, (g->B + tpw - 1) / tpw)); };
    g->gridA = split(g->gridS, EEGNET_FOLD_TPW_A);
    g->gridE = split(g->gridS, EEGNET_FOLD_TPW_E);
    g->gridS = split(g->gridS, EEGNET_FOLD_TPW_S);
    g->grid = split(g->grid, EEGNET_FOLD_TPW_C);
}

// the three launches of eegnet_ems on rows of T: chunk aggregates, carries, output; scratch holds the
// aggregates [n_rows][n_chunks][EMS_AGG], then the carries [n_rows][n_chunks][2]
template <class T>
static int ems_launch(const EmsCall& ec, const void* x, float* y, double* state, void* scratch, hipStream_t s) {
    const dim3 grid((unsigned)(ec.n_rows * ec.n_chunks));
    double* agg = (double*)scratch;
    double* carry = agg + (size_t)ec.n_rows * ec.n_chunks * EMS_AGG;
    if (int r = launch(KID_NONE, "k_ems_agg", k_ems_agg<T>, grid, dim3(EMS_NT), 0, s, ec, (const T*)x, agg)) return r;
    if (int r = launch(KID_NONE, "k_ems_carry", k_ems_carry<T>, dim3((unsigned)ec.n_rows), dim3(EMS_NTC), 0, s, ec,
                       (const T*)x, agg, carry, state)) return r;
    return launch(KID_NONE, "k_ems_out", k_ems_out<T>, grid, dim3(EMS_NT), 0, s, ec, (const T*)x, carry, y);
}

constexpr int64_t FIR_MAX_GRID = 2147483647;          // hipLaunchKernel's grid.x

// the two launches of eegnet_fir on rows of T: the outputs (when there are any), then the next history
template <class T>
static int fir_launch(const FirCall& fc, const void* x, const double* taps, const double* hist_in, double* hist_out,
                      float* y, hipStream_t s) {
    if (fc.n_out > 0)
        if (int r = launch(KID_NONE, "k_fir", k_fir<T>, dim3((unsigned)(fc.n_rows * fc.n_chunks)), dim3(FIR_NT),
                           (size_t)fir_lds_doubles(fc.L) * sizeof(double), s, fc, (const T*)x, taps, hist_in, y)) return r;
    const long long nh = fc.n_rows * (long long)(fc.L - 1);
    if (!hist_out || nh == 0) return 0;
    return launch(KID_NONE, "k_fir_hist", k_fir_hist<T>, dim3((unsigned)((nh + FIR_NT - 1) / FIR_NT)), dim3(FIR_NT), 0, s,
                  fc, (const T*)x, hist_in, hist_out);
}

// [a, a + na) and [b, b + nb) share a byte
static bool bytes_overlap(const void* a, double na, const void* b, double nb) {
    const double a0 = (double)(uintptr_t)a, b0 = (double)(uintptr_t)b;
    return a && b && na > 0 && nb > 0 && a0 < b0 + nb && b0 < a0 + na;
}

// The integers of an eegnet_resample call: the reduced ratio, the filter's geometry, the call's first output
// and its count.  Everything eegnet_resample_count answers, so nothing here looks at a pointer.
//   done(t)   outputs whose whole support lies in the first t samples: m down + half < t up
//   all(t)    outputs of a recording of t samples: ceil(t up / down)
static int rs_plan(int64_t n_samples, int64_t n_before, int n_taps, int up, int down, int mode, RsCall* rc) {
    if (mode < EEGNET_RESAMPLE_WHOLE || mode > EEGNET_RESAMPLE_TAIL)
        return fail(EEGNET_EINVAL, "eegnet_resample: unknown mode %d", mode);
    if (n_taps < 1 || n_taps > RS_MAX_TAPS || (n_taps & 1) == 0)
        return fail(EEGNET_EINVAL, "eegnet_resample: n_taps must be odd and in [1, %d] (got %d)", RS_MAX_TAPS, n_taps);
    if (up < 1 || down < 1)
        return fail(EEGNET_EINVAL, "eegnet_resample: up and down must be >= 1 (got %d/%d)", up, down);
    int a = up, b = down;
    while (b) { const int t = a % b; a = b; b = t; }
    const int u = up / a, d = down / a;
    if (u == d) return fail(EEGNET_EINVAL, "eegnet_resample: %d/%d reduces to 1/1: nothing to resample", up, down);
    if (u > RS_MAX_UP || d > RS_MAX_DOWN)
        return fail(EEGNET_EINVAL, "eegnet_resample: %d/%d reduces to %d/%d, beyond up <= %d, down <= %d", up, down, u,
                    d, RS_MAX_UP, RS_MAX_DOWN);
    const int half = (n_taps - 1) / 2, Q = half / u;
    const int64_t n_cap = ((int64_t)1 << 61) / std::max(u, d);
    if (n_before < 0 || n_before > n_cap)
        return fail(EEGNET_EINVAL, "eegnet_resample: n_before must be in [0, %lld] (got %lld)", (long long)n_cap,
                    (long long)n_before);
    const bool opens = mode == EEGNET_RESAMPLE_WHOLE || mode == EEGNET_RESAMPLE_FIRST;
    if (opens && n_before != 0)
        return fail(EEGNET_EINVAL, "eegnet_resample: a recording's first samples come after none (n_before = %lld)",
                    (long long)n_before);
    if (!opens && n_before < Q + 2)
        return fail(EEGNET_EINVAL, "eegnet_resample: a stream's first block holds at least %d samples (n_before = %lld)",
                    Q + 2, (long long)n_before);
    const int64_t n_min = mode == EEGNET_RESAMPLE_FIRST ? Q + 2 : 1;
    if (mode == EEGNET_RESAMPLE_TAIL) {
        if (n_samples != 0)
            return fail(EEGNET_EINVAL, "eegnet_resample: the tail call takes no samples (n_samples = %lld)",
                        (long long)n_samples);
    } else if (n_samples < n_min || n_samples > n_cap - n_before) {
        return fail(EEGNET_EINVAL, "eegnet_resample: n_samples must be in [%lld, %lld]%s (got %lld)", (long long)n_min,
                    (long long)(n_cap - n_before), mode == EEGNET_RESAMPLE_FIRST ? ", at least half / up + 2 for a "
                    "stream's first block" : "", (long long)n_samples);
    }
    const auto done = [&](int64_t t) { const int64_t v = t * u - half - 1; return v >= 0 ? v / d + 1 : (int64_t)0; };
    const auto all = [&](int64_t t) { return (t * u + d - 1) / d; };
    const int64_t end = n_before + n_samples;
    rc->n = n_samples;
    rc->t0 = n_before;
    rc->m_lo = opens ? 0 : done(n_before);
    rc->n_out = (mode == EEGNET_RESAMPLE_WHOLE || mode == EEGNET_RESAMPLE_TAIL ? all(end) : done(end)) - rc->m_lo;
    rc->L = n_taps;
    rc->half = half;
    rc->up = u;
    rc->down = d;
    rc->K = (n_taps + u - 1) / u;
    rc->H = 2 * Q + 2;
    rc->head_ext = opens;
    rc->tail_ext = mode == EEGNET_RESAMPLE_WHOLE || mode == EEGNET_RESAMPLE_TAIL;
    // a stream's recording holds at least Q + 2 samples (its first block does): both ends reflect Q + 1
    rc->refl = mode == EEGNET_RESAMPLE_WHOLE ? std::min<int64_t>(Q + 1, n_samples - 1) : Q + 1;
    rc->share = RS_NT % u == 0;
    // the chunk: the most outputs, up to RS_CH, whose span fits beside the table; whole workgroups' worth when
    // there is room for that.  The outputs do not depend on it.
    const long long room = LDS_MAX / 8 - (long long)rc->K * u - 1 - rc->K;
    if (room < 0)
        return fail(EEGNET_EINVAL, "eegnet_resample: %d taps at up = %d do not fit the LDS beside one output's span",
                    n_taps, u);
    long long ch = std::min<long long>(RS_CH, ((room + 1) * u - 1) / d + 1);
    if (ch >= RS_NT) ch -= ch % RS_NT;
    rc->ch = (int)ch;
    rc->n_chunks = rc->n_out > 0 ? (rc->n_out - 1) / ch + 1 : 0;
    return 0;
}

// the two launches of eegnet_resample on rows of T: the outputs (when there are any), then the next history
template <class T>
static int rs_launch(const RsCall& rc, const void* x, const double* taps, const double* hist_in, double* hist_out,
                     float* y, hipStream_t s) {
    if (rc.n_out > 0) {
        const size_t lds = ((size_t)rc.K * rc.up + (size_t)rs_span_doubles(rc.ch, rc.up, rc.down, rc.K)) * sizeof(double);
        if (int r = launch(KID_NONE, "k_resample", k_resample<T>, dim3((unsigned)(rc.n_rows * rc.n_groups)), dim3(RS_NT),
                           lds, s, rc, (const T*)x, taps, hist_in, y)) return r;
    }
    const long long nh = rc.n_rows * (long long)rc.H;
    if (!hist_out) return 0;
    return launch(KID_NONE, "k_resample_hist", k_resample_hist<T>, dim3((unsigned)((nh + RS_NT - 1) / RS_NT)), dim3(RS_NT),
                  0, s, rc, (const T*)x, hist_in, hist_out);
}

extern "C" {

int eegnet_train_step_folds(const eegnet_dims* dims, int nfolds, const eegnet_fold* folds, int64_t row0,
                            int64_t slot, uint64_t offset, float lr, float beta1, float beta2, float eps,
                            void* stream) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (g.wide) return fail(EEGNET_EINVAL, "eegnet_train_step_folds: F1*D = %d > 16 is not supported", g.F2);
    StepCall c(g, nullptr, stream);                   // no workspace: every per-fold pointer comes from `folds`
    if (int r = fold_call(&c.fc, nfolds, folds, row0, slot, offset, lr, beta1, beta2, eps)) return r;
    c.fc.off = c.off;                                 // (laid out for the non-fold grids, fold_grids' caps)
    c.nf = nfolds;
    c.c_mode = PC_BWD | PC_CE;
    set_key(&g, 0, offset);                           // the keep threshold (keys come per fold)
    ensure_attrs();
    fold_grids(&g);
    if (int r = run_forward(g, c)) return r;
    return run_backward(g, c);
}

int eegnet_eval_folds(const eegnet_dims* dims, int nfolds, const eegnet_eval_fold* folds, int64_t max_n,
                      int batch, int64_t slot, void* stream) {
    if (!dims) return fail(EEGNET_EINVAL, "dims is NULL");
    eegnet_dims d = *dims;
    d.B = 1;                                          // dims->B is ignored: the table carries every fold's n
    Geo g;
    if (int r = make_geo_narrow(&d, &g, "eegnet_eval_folds")) return r;
    if (g.XP != g.T) return fail(EEGNET_EINVAL, "eegnet_eval_folds takes x as [n][C][T] (x_pitch 0 or T)");
    if (nfolds < 1) return fail(EEGNET_EINVAL, "nfolds must be >= 1 (got %d)", nfolds);
    if (!folds) return fail(EEGNET_EINVAL, "folds is NULL");
    if (max_n < 0) return fail(EEGNET_EINVAL, "max_n must be >= 0 (got %lld)", (long long)max_n);
    if (batch < 1) return fail(EEGNET_EINVAL, "batch must be >= 1 (got %d)", batch);
    if (max_n > (int64_t)1 << 31) return fail(EEGNET_EINVAL, "max_n must be <= 2^31 (got %lld)", (long long)max_n);
    if (slot < 0) return fail(EEGNET_EINVAL, "slot must be >= 0");
    if ((g.ldsI + NCLS) * 4 > LDS_MAX)
        return fail(EEGNET_EINVAL, "eegnet_eval_folds: dims need %d B of LDS (> %d)", (g.ldsI + NCLS) * 4, LDS_MAX);
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    EvalCall ec;
    ec.folds = folds;
    ec.max_n = max_n;
    ec.total = (long long)nfolds * max_n;
    ec.slot = slot;
    ec.batch = batch;
    if (ec.total > 0) {
        // a flat grid over the (fold, trial) pairs: at most one workgroup per CU, a contiguous range each
        const long long G = std::min<long long>(device_cus(), ec.total);
        ec.chunk = (ec.total + G - 1) / G;
        const unsigned grid = (unsigned)((ec.total + ec.chunk - 1) / ec.chunk);
        if (int r = dispatch_shape(g, [&](auto sh) {
                return launch(KID_NONE, "k_eval_folds", k_eval_folds<SHAPE_OF(sh)>, dim3(grid), dim3(NTH),
                              (g.ldsI + NCLS) * 4, s, g, ec);
            })) return r;
    } else {
        ec.chunk = 1;
    }
    return launch(KID_NONE, "k_eval_folds_reduce", k_eval_folds_reduce, dim3((unsigned)nfolds), dim3(NTER), 0, s, ec);
}

// W = (n_samples - T) / hop + 1 of a recording, with the checks both window entry points share
static int window_count(const Geo& g, int64_t n_samples, int64_t hop, int64_t* W) {
    if (hop < 1) return fail(EEGNET_EINVAL, "sliding windows: hop must be >= 1 (got %lld)", (long long)hop);
    if (n_samples < g.T)
        return fail(EEGNET_EINVAL, "sliding windows: n_samples = %lld is shorter than one window (T = %d)",
                    (long long)n_samples, g.T);
    *W = (n_samples - g.T) / hop + 1;
    return 0;
}

int eegnet_window_count(const eegnet_dims* dims, int64_t n_samples, int64_t hop, int64_t* out) {
    if (!dims) return fail(EEGNET_EINVAL, "dims is NULL");
    eegnet_dims d = *dims;
    d.B = 1;                                          // dims->B is ignored: the count is per recording
    Geo g;
    if (int r = make_geo(&d, &g, false)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    return window_count(g, n_samples, hop, out);
}

int eegnet_forward_eval_windows(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                                const float* rec, int64_t n_rec, int64_t n_samples, int64_t pitch, int64_t hop,
                                float* logits, float* probs, int32_t* pred, void* stream) {
    if (!dims) return fail(EEGNET_EINVAL, "dims is NULL");
    eegnet_dims d = *dims;
    d.B = 1;                                          // dims->B is ignored: n_rec and the window count size the call
    Geo g;
    if (int r = make_geo_narrow(&d, &g, "sliding windows")) return r;
    if (g.XP != g.T) return fail(EEGNET_EINVAL, "sliding windows: x_pitch must be 0 or T (the rows' pitch is `pitch`)");
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(rec, "rec", logits, "logits")) return r;
    if (n_rec < 1) return fail(EEGNET_EINVAL, "sliding windows: n_rec must be >= 1 (got %lld)", (long long)n_rec);
    int64_t W = 0;
    if (int r = window_count(g, n_samples, hop, &W)) return r;
    if (pitch < n_samples)
        return fail(EEGNET_EINVAL, "sliding windows: pitch = %lld is below n_samples = %lld", (long long)pitch,
                    (long long)n_samples);
    // every window is one trial of the eval forward: the total must be a batch eegnet_forward_eval takes
    const double total_d = (double)n_rec * (double)W;
    if (total_d > 2147483647.0)
        return fail(EEGNET_EINVAL, "sliding windows: n_rec * W = %.0f windows exceed the batch the eval forward takes",
                    total_d);
    d.B = (int)(n_rec * W);
    if (make_geo(&d, &g)) {
        const std::string why = g_err;
        return fail(EEGNET_EINVAL, "sliding windows: n_rec * W = %d windows exceed the batch the eval forward takes (%s)",
                    d.B, why.c_str());
    }
    WinCall wc;
    wc.rec = rec;
    wc.pitch = pitch;
    wc.hop = hop;
    wc.W = (int)W;
    wc.total = d.B;
    // 16-byte loads only when every window row starts 16-byte aligned
    wc.vec = (g.T & 3) == 0 && (hop & 3) == 0 && (pitch & 3) == 0 && ((uintptr_t)rec & 15) == 0;
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    if (int r = dispatch_shape(g, [&](auto sh) {
            return launch(KID_NONE, "k_infer_win", k_infer_win<SHAPE_OF(sh)>, dim3(g.grid), dim3(NTH), g.ldsI * 4, s, g,
                          params, bn_buffers, wc, logits);
        })) return r;
    if (!probs && !pred) return 0;
    return launch(KID_NONE, "k_win_reduce", k_win_reduce, dim3((unsigned)n_rec), dim3(NTWR), 0, s, logits, wc.W, probs,
                  pred);
}

int eegnet_forward_eval_windows_at(const eegnet_dims* dims, const float* params, const float* bn_buffers,
                                   const float* rec, int64_t n_rec, int64_t n_samples, int64_t pitch,
                                   const int64_t* starts, const int32_t* rec_index, int64_t n_windows, float* logits,
                                   void* stream) {
    if (!dims) return fail(EEGNET_EINVAL, "dims is NULL");
    eegnet_dims d = *dims;
    d.B = 1;                                          // dims->B is ignored: the table sizes the call
    Geo g;
    if (int r = make_geo_narrow(&d, &g, "windows at a table")) return r;
    if (g.XP != g.T) return fail(EEGNET_EINVAL, "windows at a table: x_pitch must be 0 or T (the rows' pitch is `pitch`)");
    if (int r = check_ptrs(params, "params", bn_buffers, "bn_buffers")) return r;
    if (int r = check_ptrs(rec, "rec", logits, "logits")) return r;
    if (int r = check_ptrs(starts, "starts")) return r;
    if (n_rec < 1 || n_rec > 2147483647)
        return fail(EEGNET_EINVAL, "windows at a table: n_rec must be in [1, 2^31) (got %lld)", (long long)n_rec);
    if (n_samples < g.T)
        return fail(EEGNET_EINVAL, "windows at a table: n_samples = %lld is shorter than one window (T = %d)",
                    (long long)n_samples, g.T);
    if (pitch < n_samples)
        return fail(EEGNET_EINVAL, "windows at a table: pitch = %lld is below n_samples = %lld", (long long)pitch,
                    (long long)n_samples);
    if (((uintptr_t)rec & 3) || ((uintptr_t)starts & 7) || ((uintptr_t)rec_index & 3))
        return fail(EEGNET_EINVAL, "windows at a table: rec, starts and rec_index must be aligned to their element size");
    if (n_windows < 1 || n_windows > 2147483647)
        return fail(EEGNET_EINVAL, "windows at a table: n_windows must be in [1, 2^31) (got %lld)", (long long)n_windows);
    d.B = (int)n_windows;                             // every window is one trial of the eval forward
    if (make_geo(&d, &g)) {
        const std::string why = g_err;
        return fail(EEGNET_EINVAL, "windows at a table: %d windows exceed the batch the eval forward takes (%s)", d.B,
                    why.c_str());
    }
    WinAtCall ac;
    ac.rec = rec;
    ac.pitch = pitch;
    ac.hop = 0;
    ac.W = 0;
    ac.total = d.B;
    ac.vec = 0;
    ac.starts = (const long long*)starts;
    ac.rec_index = rec_index;
    ac.last = n_samples - g.T;
    ac.n_rec = (int)n_rec;
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    return dispatch_shape(g, [&](auto sh) {
        return launch(KID_NONE, "k_infer_win(at)", k_infer_win<SHAPE_OF(sh), WinAtCall>, dim3(g.grid), dim3(NTH),
                      g.ldsI * 4, s, g, params, bn_buffers, ac, logits);
    });
}

int eegnet_fir_max_taps(void) { return FIR_MAX_TAPS; }

int eegnet_fir_chunk(void) { return FIR_CH; }

int eegnet_fir(const void* x, int x_is_f64, int64_t n_rows, int64_t n_samples, int64_t x_pitch, const double* taps,
               int n_taps, float* y, int64_t y_pitch, const double* hist_in, double* hist_out, int mode, void* stream) {
    if (mode < EEGNET_FIR_WHOLE || mode > EEGNET_FIR_TAIL)
        return fail(EEGNET_EINVAL, "eegnet_fir: unknown mode %d", mode);
    if (mode != EEGNET_FIR_TAIL)
        if (int r = check_ptrs(x, "x")) return r;
    if (int r = check_ptrs(y, "y", taps, "taps")) return r;
    if (n_taps < 1 || n_taps > FIR_MAX_TAPS)
        return fail(EEGNET_EINVAL, "eegnet_fir: n_taps must be in [1, %d] (got %d)", FIR_MAX_TAPS, n_taps);
    if (mode != EEGNET_FIR_NEXT && (n_taps & 1) == 0)
        return fail(EEGNET_EINVAL, "eegnet_fir: a zero-phase filter needs an odd n_taps (got %d); only a continuation "
                    "call takes an even one", n_taps);
    const int L = n_taps, M = (L - 1) / 2;
    if (n_rows < 1) return fail(EEGNET_EINVAL, "eegnet_fir: n_rows must be >= 1 (got %lld)", (long long)n_rows);
    const int64_t n_min = mode == EEGNET_FIR_FIRST ? L : 1;
    if (mode == EEGNET_FIR_TAIL) {
        if (n_samples != 0)
            return fail(EEGNET_EINVAL, "eegnet_fir: the tail call takes no samples (n_samples = %lld)", (long long)n_samples);
    } else if (n_samples < n_min) {
        return fail(EEGNET_EINVAL, "eegnet_fir: n_samples must be >= %lld%s (got %lld)", (long long)n_min,
                    mode == EEGNET_FIR_FIRST ? " = n_taps for a stream's first block" : "", (long long)n_samples);
    }
    const bool need_in = (mode == EEGNET_FIR_NEXT || mode == EEGNET_FIR_TAIL) && L > 1;
    const bool need_out = (mode == EEGNET_FIR_FIRST || mode == EEGNET_FIR_NEXT) && L > 1;
    if (need_in && !hist_in) return fail(EEGNET_EINVAL, "eegnet_fir: this mode reads the history: hist_in is NULL");
    if (need_out && !hist_out) return fail(EEGNET_EINVAL, "eegnet_fir: this mode writes the history: hist_out is NULL");
    FirCall fc;
    fc.n_rows = n_rows;
    fc.n = n_samples;
    fc.L = L;
    fc.M = M;
    fc.head_reflect = mode == EEGNET_FIR_WHOLE || mode == EEGNET_FIR_FIRST;
    fc.tail_reflect = mode == EEGNET_FIR_WHOLE || mode == EEGNET_FIR_TAIL;
    fc.t_lo = fc.head_reflect ? 0 : -M;
    fc.n_out = mode == EEGNET_FIR_WHOLE ? n_samples : mode == EEGNET_FIR_FIRST ? n_samples - M
               : mode == EEGNET_FIR_NEXT ? n_samples : M;
    // a stream's recording holds at least n_taps samples (its first block does): both ends reflect M
    fc.refl = mode == EEGNET_FIR_WHOLE ? std::min<int64_t>(M, n_samples - 1) : M;
    fc.n_chunks = fc.n_out > 0 ? (fc.n_out - 1) / FIR_CH + 1 : 0;
    if (fc.n_chunks > FIR_MAX_GRID / n_rows || (int64_t)(L - 1) > FIR_MAX_GRID / n_rows * FIR_NT)
        return fail(EEGNET_EINVAL, "eegnet_fir: n_rows = %lld rows of %lld chunks (%d outputs each) exceed the grid limit "
                    "of %lld workgroups", (long long)n_rows, (long long)fc.n_chunks, FIR_CH, (long long)FIR_MAX_GRID);
    if (mode != EEGNET_FIR_TAIL && x_pitch < n_samples)
        return fail(EEGNET_EINVAL, "eegnet_fir: x_pitch = %lld is below n_samples = %lld", (long long)x_pitch,
                    (long long)n_samples);
    if (y_pitch < fc.n_out)
        return fail(EEGNET_EINVAL, "eegnet_fir: y_pitch = %lld is below the %lld outputs of a row", (long long)y_pitch,
                    (long long)fc.n_out);
    fc.x_pitch = x_pitch;
    fc.y_pitch = y_pitch;
    const uintptr_t xa = x_is_f64 ? 7 : 3;
    if (((uintptr_t)x & xa) || ((uintptr_t)y & 3) || ((uintptr_t)taps & 7) || ((uintptr_t)hist_in & 7) ||
        ((uintptr_t)hist_out & 7))
        return fail(EEGNET_EINVAL, "eegnet_fir: x, y, taps and the histories must be aligned to their element size");
    // a workgroup's outputs would overwrite inputs its neighbours still read: no in-place filtering.  The
    // extents are the rows' bounding ranges, first byte of the first row to last byte of the last.
    const double xb = ((double)(n_rows - 1) * (double)x_pitch + (double)n_samples) * (x_is_f64 ? 8.0 : 4.0);
    const double yb = ((double)(n_rows - 1) * (double)y_pitch + (double)fc.n_out) * 4.0;
    const double hb = (double)n_rows * (double)(L - 1) * 8.0;
    if (mode != EEGNET_FIR_TAIL && bytes_overlap(x, xb, y, yb))
        return fail(EEGNET_EINVAL, "eegnet_fir: y overlaps x (filtering in place is not supported)");
    if (need_in && need_out && bytes_overlap(hist_in, hb, hist_out, hb))
        return fail(EEGNET_EINVAL, "eegnet_fir: hist_out overlaps hist_in (the call reads one and writes the other)");
    if (!need_in) hist_in = nullptr;
    if (!need_out) hist_out = nullptr;
    if (fc.n_out == 0 && !hist_out) return 0;          // (the tail of a one-tap filter)
    hipStream_t s = (hipStream_t)stream;
    return x_is_f64 ? fir_launch<double>(fc, x, taps, hist_in, hist_out, y, s)
                    : fir_launch<float>(fc, x, taps, hist_in, hist_out, y, s);
}

int eegnet_resample_max_taps(void) { return RS_MAX_TAPS; }

int eegnet_resample_max_up(void) { return RS_MAX_UP; }

int eegnet_resample_chunk(int n_taps, int up, int down) {
    RsCall rc;
    if (int r = rs_plan(1, 0, n_taps, up, down, EEGNET_RESAMPLE_WHOLE, &rc)) return r;
    return rc.ch;
}

int eegnet_resample_count(int64_t n_samples, int64_t n_before, int n_taps, int up, int down, int mode, int64_t* n_out) {
    if (int r = check_ptrs(n_out, "n_out")) return r;
    RsCall rc;
    if (int r = rs_plan(n_samples, n_before, n_taps, up, down, mode, &rc)) return r;
    *n_out = rc.n_out;
    return 0;
}

int eegnet_resample(const void* x, int x_is_f64, int64_t n_rows, int64_t n_samples, int64_t x_pitch, const double* taps,
                    int n_taps, int up, int down, int ends, float* y, int64_t y_pitch, int64_t n_before,
                    const double* hist_in, double* hist_out, int mode, void* stream) {
    RsCall rc;
    if (int r = rs_plan(n_samples, n_before, n_taps, up, down, mode, &rc)) return r;
    if (mode != EEGNET_RESAMPLE_TAIL)
        if (int r = check_ptrs(x, "x")) return r;
    if (int r = check_ptrs(taps, "taps")) return r;
    if (rc.n_out > 0)                                   // (a continuation too short for an output writes none)
        if (int r = check_ptrs(y, "y")) return r;
    if (ends != EEGNET_RESAMPLE_ENDS_ZERO && ends != EEGNET_RESAMPLE_ENDS_REFLECT)
        return fail(EEGNET_EINVAL, "eegnet_resample: unknown ends %d", ends);
    if (n_rows < 1) return fail(EEGNET_EINVAL, "eegnet_resample: n_rows must be >= 1 (got %lld)", (long long)n_rows);
    const bool need_in = mode == EEGNET_RESAMPLE_NEXT || mode == EEGNET_RESAMPLE_TAIL;
    const bool need_out = mode == EEGNET_RESAMPLE_FIRST || mode == EEGNET_RESAMPLE_NEXT;
    if (need_in && !hist_in) return fail(EEGNET_EINVAL, "eegnet_resample: this mode reads the history: hist_in is NULL");
    if (need_out && !hist_out) return fail(EEGNET_EINVAL, "eegnet_resample: this mode writes the history: hist_out is NULL");
    rc.n_rows = n_rows;
    rc.reflect = ends == EEGNET_RESAMPLE_ENDS_REFLECT;
    if (rc.n_chunks > FIR_MAX_GRID / n_rows || (int64_t)rc.H > FIR_MAX_GRID / n_rows * RS_NT)
        return fail(EEGNET_EINVAL, "eegnet_resample: n_rows = %lld rows of %lld chunks (%d outputs each) exceed the grid "
                    "limit of %lld workgroups", (long long)n_rows, (long long)rc.n_chunks, rc.ch, (long long)FIR_MAX_GRID);
    // a workgroup stages the table once and runs up to RS_CPW chunks under it, while that leaves the chip
    // RS_MIN_GRID workgroups to spread
    rc.cpw = (int)std::max<int64_t>(1, std::min<int64_t>(RS_CPW, n_rows * rc.n_chunks / RS_MIN_GRID));
    rc.n_groups = (rc.n_chunks + rc.cpw - 1) / rc.cpw;
    if (mode != EEGNET_RESAMPLE_TAIL && x_pitch < n_samples)
        return fail(EEGNET_EINVAL, "eegnet_resample: x_pitch = %lld is below n_samples = %lld", (long long)x_pitch,
                    (long long)n_samples);
    if (y_pitch < rc.n_out)
        return fail(EEGNET_EINVAL, "eegnet_resample: y_pitch = %lld is below the %lld outputs of a row", (long long)y_pitch,
                    (long long)rc.n_out);
    rc.x_pitch = x_pitch;
    rc.y_pitch = y_pitch;
    const uintptr_t xa = x_is_f64 ? 7 : 3;
    if (((uintptr_t)x & xa) || ((uintptr_t)y & 3) || ((uintptr_t)taps & 7) || ((uintptr_t)hist_in & 7) ||
        ((uintptr_t)hist_out & 7))
        return fail(EEGNET_EINVAL, "eegnet_resample: x, y, taps and the histories must be aligned to their element size");
    // a workgroup's outputs would overwrite inputs its neighbours still read: no resampling in place
    const double xb = ((double)(n_rows - 1) * (double)x_pitch + (double)n_samples) * (x_is_f64 ? 8.0 : 4.0);
    const double yb = ((double)(n_rows - 1) * (double)y_pitch + (double)rc.n_out) * 4.0;
    const double hb = (double)n_rows * (double)rc.H * 8.0;
    if (mode != EEGNET_RESAMPLE_TAIL && bytes_overlap(x, xb, y, yb))
        return fail(EEGNET_EINVAL, "eegnet_resample: y overlaps x (resampling in place is not supported)");
    if (need_in && need_out && bytes_overlap(hist_in, hb, hist_out, hb))
        return fail(EEGNET_EINVAL, "eegnet_resample: hist_out overlaps hist_in (the call reads one and writes the other)");
    if (!need_in) hist_in = nullptr;
    if (!need_out) hist_out = nullptr;
    if (rc.n_out == 0 && !hist_out) return 0;
    ensure_attrs();
    hipStream_t s = (hipStream_t)stream;
    return x_is_f64 ? rs_launch<double>(rc, x, taps, hist_in, hist_out, y, s)
                    : rs_launch<float>(rc, x, taps, hist_in, hist_out, y, s);
}

// chunks per row and workgroups of an eegnet_ems call; the sizes are checked before anything is multiplied
constexpr int64_t EMS_MAX_GRID = 2147483647;          // hipLaunchKernel's grid.x
static int ems_sizes(int64_t n_rows, int64_t n_samples, int64_t* n_chunks) {
    if (n_rows < 1) return fail(EEGNET_EINVAL, "eegnet_ems: n_rows must be >= 1 (got %lld)", (long long)n_rows);
    if (n_samples < 1) return fail(EEGNET_EINVAL, "eegnet_ems: n_samples must be >= 1 (got %lld)", (long long)n_samples);
    const int64_t nc = (n_samples - 1) / EMS_L + 1;
    if (nc > EMS_MAX_GRID / n_rows)
        return fail(EEGNET_EINVAL, "eegnet_ems: n_rows = %lld rows of %lld chunks (%d samples each) exceed the grid "
                    "limit of %lld workgroups", (long long)n_rows, (long long)nc, EMS_L, (long long)EMS_MAX_GRID);
    *n_chunks = nc;
    return 0;
}

int eegnet_ems_chunk(void) { return EMS_L; }

int eegnet_ems_scratch_bytes(int64_t n_rows, int64_t n_samples, size_t* out) {
    int64_t nc = 0;
    if (int r = ems_sizes(n_rows, n_samples, &nc)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    *out = (size_t)n_rows * (size_t)nc * (EMS_AGG + 2) * sizeof(double);      // aggregates, then carries
    return 0;
}

int eegnet_ems(const void* x, int x_is_f64, int64_t n_rows, int64_t n_samples, int64_t x_pitch, float* y,
               int64_t y_pitch, double factor_new, int64_t init_block, double eps, double* state, int resume,
               void* scratch, void* stream) {
    if (int r = check_ptrs(x, "x", y, "y")) return r;
    if (int r = check_ptrs(scratch, "scratch")) return r;
    int64_t n_chunks = 0;
    if (int r = ems_sizes(n_rows, n_samples, &n_chunks)) return r;
    if (x_pitch < n_samples)
        return fail(EEGNET_EINVAL, "eegnet_ems: x_pitch = %lld is below n_samples = %lld", (long long)x_pitch,
                    (long long)n_samples);
    if (y_pitch < n_samples)
        return fail(EEGNET_EINVAL, "eegnet_ems: y_pitch = %lld is below n_samples = %lld", (long long)y_pitch,
                    (long long)n_samples);
    if (!(factor_new > 0.0 && factor_new < 1.0))
        return fail(EEGNET_EINVAL, "eegnet_ems: factor_new must lie in (0, 1) (got %g)", factor_new);
    if (!(eps >= 0.0)) return fail(EEGNET_EINVAL, "eegnet_ems: eps must be >= 0 (got %g)", eps);
    if (resume) {
        if (!state) return fail(EEGNET_EINVAL, "eegnet_ems: resume needs state");
    } else if (init_block < 1) {
        return fail(EEGNET_EINVAL, "eegnet_ems: init_block must be >= 1 (got %lld)", (long long)init_block);
    }
    if ((const void*)y == x) {
        if (x_is_f64) return fail(EEGNET_EINVAL, "eegnet_ems: y may be x for fp32 input only");
        if (y_pitch != x_pitch)
            return fail(EEGNET_EINVAL, "eegnet_ems: y is x but y_pitch = %lld is not x_pitch = %lld", (long long)y_pitch,
                        (long long)x_pitch);
    }
    const uintptr_t xa = x_is_f64 ? 7 : 3;
    if (((uintptr_t)x & xa) || ((uintptr_t)y & 3) || ((uintptr_t)scratch & 7) || ((uintptr_t)state & 7))
        return fail(EEGNET_EINVAL, "eegnet_ems: x, y, state and scratch must be aligned to their element size");
    EmsCall ec;
    ec.n_rows = n_rows;
    ec.n = n_samples;
    ec.n_chunks = n_chunks;
    ec.x_pitch = x_pitch;
    ec.y_pitch = y_pitch;
    ec.a = factor_new;
    ec.p = 1.0 - factor_new;
    ec.eps = eps;
    ec.init_n = resume ? 0 : std::min(init_block, n_samples);
    ec.resume = resume ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    return x_is_f64 ? ems_launch<double>(ec, x, y, state, scratch, s) : ems_launch<float>(ec, x, y, state, scratch, s);
}

int eegnet_launch_grids(const eegnet_dims* dims, int fold_launch, int out[6]) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (!out) return fail(EEGNET_EINVAL, "out is NULL");
    if (fold_launch) {
        if (g.wide) return fail(EEGNET_EINVAL, "eegnet_train_step_folds: F1*D = %d > 16 is not supported", g.F2);
        fold_grids(&g);
    }
    // the wide streaming passes run NOC chunk workgroups per trial range (wide_unit)
    const int noc = g.wide ? g.NOC : 1;
    out[0] = g.gridA / noc;
    out[1] = (g.wide ? grid_wpass_b(g, spec_w5(g)) : g.gridS) / noc;
    // trial streams of pass C: k_pass_c gives each of a workgroup's nwC waves its own trials (wave i of
    // workgroup r: rows r nwC + i, + grid nwC, ...); every other kernel runs a workgroup's trials in turn
    out[2] = g.wide ? g.gridW2 : g.grid * g.nwC;
    out[3] = g.wide ? g.grid : g.gridS;     // k_wpass_d, k_pass_dr
    out[4] = g.gridE / noc;
    out[5] = fold_launch ? 0 : g.grid;      // (eegnet_eval_folds splits by its fold table, not by dims)
    return 0;
}

int eegnet_x_stats_width(const eegnet_dims* dims) {
    Geo g;
    if (int r = make_geo_narrow(dims, &g, "eegnet_x_stats", false)) return r;
    return g.K1 + 1 + g.nedge;
}

int eegnet_x_stats(const eegnet_dims* dims, int64_t n, const float* x, float* out, void* stream) {
    Geo g;
    if (int r = make_geo(dims, &g)) return r;
    if (g.wide) return fail(EEGNET_EINVAL, "eegnet_x_stats: F1*D = %d > 16 is not supported", g.F2);
    if (n < 0) return fail(EEGNET_EINVAL, "n must be >= 0");
    if (n == 0) return 0;
    if (int r = check_ptrs(x, "x", out, "out")) return r;
    ensure_attrs();
    const size_t lds = (size_t)(g.C * g.RS + NWB * (g.K1 + 1)) * 4;
    if (lds > (size_t)LDS_MAX) return fail(EEGNET_EINVAL, "eegnet_x_stats: dims need %zu B of LDS", lds);
    const dim3 grid((unsigned)std::min<int64_t>(n, (int64_t)device_cus() * WGPC));
    hipStream_t s = (hipStream_t)stream;
    return dispatch_shape(g, [&](auto sh) {
        return launch(KID_XSTATS, "k_xstats", k_xstats<decltype(sh)::K1>, grid, dim3(NTB), lds, s, g, n, x, out);
    });
}

int eegnet_clamp_grads(const eegnet_dims* dims, float* grads, void* stream) {
    Geo g;
    if (int r = make_geo(dims, &g, false)) return r;
    if (!grads) return fail(EEGNET_EINVAL, "grads is NULL");
    hipStream_t s = (hipStream_t)stream;
    const int n = std::max(g.F2 * g.C, NCLS * g.NF);
    return launch(KID_NONE, "k_clamp", k_clamp, dim3((n + 255) / 256), dim3(256), 0, s, g, grads);
}

#ifdef EEGNET_TRACE
// debug hook of the traced build: workgroup 0 dumps its first trial's s [F2P,T], a [F2P,T/4] and
// z [F2P,T/4] planes (fp32) into `buf` (NULL turns it off)
int eegnet_debug_bf16(float* buf) {
    g_bf16_dbg = buf;
    return 0;
}
#endif

const char* eegnet_last_error(void) { return g_err.c_str(); }

int eegnet_trace_enable(void* buf) {
    g_trace_buf = (unsigned long long*)buf;
    return 0;
}

size_t eegnet_dims_bytes(void) { return sizeof(eegnet_dims); }
size_t eegnet_fold_bytes(void) { return sizeof(eegnet_fold); }
size_t eegnet_eval_fold_bytes(void) { return sizeof(eegnet_eval_fold); }
int eegnet_abi_version(void) { return EEGNET_ABI_VERSION; }

size_t eegnet_trace_bytes(void) { return (size_t)8 * TR_MAXWG * TR_SLOTS * sizeof(unsigned long long); }

int eegnet_profile_enable(int on) {
    g_prof.mask = (unsigned)on;
    return 0;
}

int eegnet_profile_collect(char* names, int* counts, double* total_ms, int cap, int* n_out) {
    double tot[KID_COUNT] = {0};
    int cnt[KID_COUNT] = {0};
    for (auto& r : g_prof.recs) {
        hipEventSynchronize(r.b);
        float ms = 0.f;
        hipEventElapsedTime(&ms, r.a, r.b);
        tot[r.kid] += ms;
        cnt[r.kid] += 1;
        g_prof.pool.push_back(r.a);
        g_prof.pool.push_back(r.b);
    }
    g_prof.recs.clear();
    int n = 0;
    for (int k = 0; k < KID_COUNT && n < cap; ++k) {
        if (!cnt[k]) continue;
        if (names) { strncpy(names + 32 * n, kKernelNames[k], 31); names[32 * n + 31] = 0; }
        if (counts) counts[n] = cnt[k];
        if (total_ms) total_ms[n] = tot[k];
        ++n;
    }
    if (n_out) *n_out = n;
    return 0;
}

const char* eegnet_build_info(void) {
    return "libeegnet_hip: gfx950 (CDNA4), fp32 VALU FIR/Gram + f32 MFMA 16x16x4 GEMMs, "
           "5-pass restructured EEGNet train step, 1024-thread row-per-wave workgroups, "
           "in-kernel ticketed fp64 reductions + finalize";
}

}  // extern "C"
