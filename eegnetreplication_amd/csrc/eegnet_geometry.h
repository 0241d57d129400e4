// eegnet_geometry.h -- the shape arithmetic of Geo and GeoI: every field that follows from the model dims
// (C, T, F1, D, K1) alone, as constexpr functions the host calls per launch (eegnet_host.hip make_geo,
// make_geo_bf16) and the compile-time-geometry kernels take as constants (kGeoW5, kGeoCfg5).  Included by
// eegnet_kernels.hip after the kernels, whose size helpers and workgroup constants it uses.
#pragma once

namespace eeg {

// dynamic LDS per workgroup: 160 KiB less a little room for the static LDS of the traced build
constexpr int LDS_MAX = 160 * 1024 - 256;

constexpr int rup(int a, int m) { return (a + m - 1) / m * m; }

struct ModelDims { int C, T, F1, D, K1; };
template <class G>
constexpr ModelDims model_dims(const G& g) { return {g.C, g.T, g.F1, g.D, g.K1}; }

// cfg5, EEGNet-16,4 at 64 x 512 with K1 = 32: the dims of the compile-time-geometry kernels, the SPEC
// instantiations of the wide kernels (eegnet_wide.hip) and k_infer_bf16_cfg5 (eegnet_infer_bf16c.hip)
constexpr ModelDims kDimsCfg5 = {64, 512, 16, 4, 32};
constexpr bool is_cfg5(ModelDims m) {
    return m.C == kDimsCfg5.C && m.T == kDimsCfg5.T && m.F1 == kDimsCfg5.F1 && m.D == kDimsCfg5.D && m.K1 == kDimsCfg5.K1;
}

// The compile-time shapes of the narrow (F2 <= 16) kernels, Shape<K1, CC, TT, FF>: EEGNet-FF/2,2 on CC
// electrodes x TT samples (the benchmark and real-data configurations).  The one list: dispatch_shape
// launches them, geo_shape sizes their LDS, ensure_attrs raises their LDS limit.
template <int K1_, int CC_, int TT_, int FF_>
struct Shape { static constexpr int K1 = K1_, CC = CC_, TT = TT_, FF = FF_; };
template <class... S>
struct Shapes {
    // f(S{}) for the shapes of the list in turn, until one returns true.  (A left fold, here and in
    // set_attrs_shapes: the compiler instantiates a right fold's operands last to first, and the code
    // object holds the kernels in the order of their first instantiation.)
    template <class F>
    static constexpr bool any(F&& f) { return (... || f(S{})); }
};
using NarrowShapes = Shapes<Shape<32, 22, 256, 16>, Shape<32, 22, 257, 16>>;

template <class S>
constexpr bool has_shape(ModelDims m, S) {
    return m.K1 == S::K1 && m.C == S::CC && m.T == S::TT && m.D == 2 && m.F1 == S::FF / 2;
}
constexpr bool narrow_spec(ModelDims m) {
    return NarrowShapes::any([m](auto sh) { return has_shape(m, sh); });
}
// the compile-time shape whose x loads honour a row pitch: the one whose rows are not 16-byte units
// (22 x 257, the recordings); the kernels of the others take the pitch as the compile-time T (EEG_XP)
constexpr bool x_pitch_shape(ModelDims m) {
    return NarrowShapes::any([m](auto sh) { return (decltype(sh)::TT & 3) != 0 && has_shape(m, sh); });
}

// flat parameter offsets (named_parameters order) of a Geo or GeoI whose dims and NF are set; the count
template <class G>
constexpr int param_offsets(G& g) {
    int o = 0;
    g.o_w1 = o; o += g.F1 * g.K1;
    g.o_g1 = o; o += g.F1;
    g.o_b1 = o; o += g.F1;
    g.o_ws = o; o += g.F2 * g.C;
    g.o_g2 = o; o += g.F2;
    g.o_b2 = o; o += g.F2;
    g.o_w2 = o; o += g.F2 * 16;
    g.o_W3 = o; o += g.F2 * g.F2;
    g.o_g3 = o; o += g.F2;
    g.o_b3 = o; o += g.F2;
    g.o_Wfc = o; o += NCLS * g.NF;
    g.o_bfc = o; o += NCLS;
    return o;
}

// the reduction tail and finalize reuse each pass kernel's LDS (floats; doubles = 2 floats)
constexpr int tail_floats(int ncols, int fin) { return 2 * (tail_s_doubles(ncols) + std::max(tail_scratch_doubles(ncols), fin)); }
constexpr int tailw_floats(int ncols, int fin) { return 2 * (tail_s_doubles(ncols) + fin); }

// F2 > 16: o-chunked streaming passes and whole-trial block-2 passes (eegnet_wide.hip)
constexpr void geo_shape_wide(Geo& g) {
    g.NOC = (g.F2 + 15) / 16;
    g.CPC = (g.C + g.NOC - 1) / g.NOC;
    g.F2P = g.F2 <= 32 ? 32 : 64;
    g.RB = rb_stride(g.T1);
    // partial rows wider than this reduce in k_coltail (column-parallel) instead of in-kernel
    g.splitC = g.nC > SPLIT_COLS; g.splitD = g.nD > SPLIT_COLS; g.splitE = g.nE > SPLIT_COLS;
    const int nf4 = rup(g.NF, 4);
    const int awl = KSW * 64;                               // spatial GEMM fragment table
    // after the loop pass A's Gram tiles [NWW][16][16 NWT] reuse the slice / s rows when they fit
    const int cgw = NWW * 256 * ((15 + g.K1 - 1) / 16 + 1);
    // the cfg5 shape (k_wpass_a's SPEC instantiation) double-buffers the slice and the s rows
    const bool w5 = is_cfg5(model_dims(g));
    const int baseA = (w5 ? 2 : 1) * (g.CPC + 16) * g.RS + NWW * (g.K1 + 1) + 2 * NWW + awl;
    g.ldsWA = std::max(baseA + ((g.CPC + 16) * g.RS >= cgw ? 0 : cgw),
                       tailw_floats(g.nA, std::max(NTH, fin1_scratch_doubles(g.K1, g.F1, g.F2, g.C))));
    g.ldsWB = 0;                                            // k_wpass_b: registers only (v plane)
    const int b2 = 2 * g.F2P * g.RB + g.F2P * K2 + g.F2P * (g.F2P + 1);   // D2, Q, w2, W3 tables
    // the whole-trial block-2 passes (k_wpass_b2 / c / d) at NWB2 waves
    const int TQ1 = (g.T1 + 3) / 4;
    g.ldsWB2 = std::max(b2 + NWB2 * 2 * 16, tailw_floats(g.nB, 0));
    g.ldsWC = std::max(nf4 + NWB2 * 4 + NWB2 * 2 * 16 + g.F2P * g.RB, tailw_floats(g.nC, 0));    // H | sums | XH
    g.ldsWD = std::max(b2 + g.F2P * g.RB + nf4 + 2 * g.F2 * TQ1, tailw_floats(g.nD, 0));
    // the cfg5 (SPEC) k_wpass_b2 keeps its W3 fragments in registers instead of an LDS table, and it and
    // k_wpass_c stay within 128 VGPRs: two 8-wave workgroups per CU (make_geo: gridW2)
    if (w5) g.ldsWB2 = std::max(g.ldsWB2 - g.F2P * (g.F2P + 1), tailw_floats(g.nB, 0));
    // s rows, dy / e rows x 2 (alternate trials), dp2 rows, coefficient table
    g.ldsWE = std::max(std::max(3 * 16 * g.RS + rup(16 * g.T1, 4) + 8 * 16 + awl, NWW * 256 + 32 + NWW * 256 * ((15 + g.K1 - 1) / 16 + 1)),
                       tailw_floats(g.nE, fin5_scratch_doubles(g.K1, g.F1, g.o_g2)));
    g.ldsWI = 16 * g.RS + b2 + nf4 + 4 * g.F2P + g.NOC * awl;
}

// Every field of Geo that follows from the (validated) model dims; the rest -- B, the dropout and BatchNorm
// arguments, the grids, pointers -- stays zero for make_geo.
constexpr Geo geo_shape(ModelDims m) {
    Geo g{};
    g.C = m.C; g.T = m.T; g.F1 = m.F1; g.D = m.D; g.K1 = m.K1;
    g.F2 = g.F1 * g.D;
    g.P = (g.K1 - 1) / 2; g.R = g.K1 - 1 - g.P;
    g.T1 = g.T / 4; g.T2 = g.T1 / 8; g.NF = g.F2 * g.T2;
    g.LP = (g.R + 3) & ~3;
    g.TQ = (g.T + 3) / 4; g.NT16 = (g.T + 15) / 16; g.NKG = g.NT16;
    g.RS = row_stride(g.K1, g.T);
    g.RS2 = rup(LP2 + g.T1 + 8, 4);
    g.CK = rup(g.C, 4); g.NCT = (g.C + 15) / 16;
    g.nH = g.R * (g.R + 1) / 2;
    g.nTl = g.P * (g.P + 1) / 2;
    g.nedge = g.nH + g.nTl + g.R + g.P;
    g.nparam = param_offsets(g);
    g.nA = g.K1 + 1 + g.nedge + 2 * g.F2;
    g.nB = 2 * g.F2;
    g.nC = NCLS * g.NF + NCLS + 2 * g.F2 + 1;
    g.nD = g.F2 * g.F2 + 18 * g.F2;
    g.QR = (g.F2 <= F2MAX && g.D == 2) ? g.F1 : g.F2;
    g.nE = g.QR * g.K1 + g.F2 * g.C + 2 * g.F2;
    const int rows1 = g.C * g.RS;                   // x rows (one buffer)
    const int nf4 = rup(g.NF, 4);
    const bool spec = narrow_spec(m);
    // compile-time shapes: two x buffers, and two xstat-row slots (fold launches, eegnet_fold.xstat)
    g.ldsA = (spec ? 2 : 1) * rows1 + g.F2 * g.RS + NWB * (g.K1 + 1) + (spec ? 2 * rup(g.K1 + 1 + g.nedge, 4) : 0);
    g.ldsB = 3 * g.F2 * g.RS2 + F2MAX * (K2 + F2MAX);
    // pass C: one trial stream per wave, each with its own row of head features
    const int pwC = nf4;
    g.nwC = std::max(1, std::min(spec ? NWAVE : NTHS / 64, (LDS_MAX / 4 - 4 * F2MAX) / pwC));
    g.ldsC = std::max(g.nwC * pwC + 4 * F2MAX, g.nwC * g.nC);   // Hs rows + the BN3 constant table
    g.ldsD = std::max(dr_lds_floats(spec ? 1 : MAXT1Q), dr_tail_floats(spec));     // k_pass_dr
    g.ldsE = std::max((2 * g.F2 + g.C) * g.RS + rup(g.F2 * g.T1, 4) + 8 * g.F2,
                      NWB * 256 * (1 + (15 + g.K1 - 1) / 16 + 1));   // after the loop: dws, Cq tiles
    // the whole-trial kernels carve trial_lds (eegnet_trial.hip): ldsI is its plain plan without the logits
    // (k_infer; k_eval_folds launches with ldsI + NCLS), ldsX its PLANE plan with them (k_infer_dx, k_frozen;
    // checked by check_lds_x alone)
    g.ldsI = trial_lds(g.C, g.F2, g.RS, g.RS2, g.NF, false).Lg;
    g.ldsX = trial_lds(g.C, g.F2, g.RS, g.RS2, g.NF, true).n;
    g.ldsA = std::max(g.ldsA, tail_floats(g.nA, fin1_scratch_doubles(g.K1, g.F1, g.F2, g.C)));
    g.ldsB = std::max(g.ldsB, tail_floats(g.nB, 0));
    g.ldsC = std::max(g.ldsC, tail_floats(g.nC, 0));
    g.ldsD = std::max(g.ldsD, tail_floats(g.nD, 0));
    g.ldsE = std::max(g.ldsE, tail_floats(g.nE, fin5_scratch_doubles(g.K1, g.F1, g.o_g2)));
    g.wide = g.F2 > F2MAX ? 1 : 0;
    if (g.wide) geo_shape_wide(g);
    return g;
}

// The geometry the SPEC instantiations of the wide kernels are compiled for.  The host launches them for
// exactly these dims (spec_w5), and geo_w<true> overwrites the fields named in EEG_FIELDS_W5
// (eegnet_common.h) with these values, which make_geo computes for the generic path by the same function.
constexpr Geo kGeoW5 = geo_shape(kDimsCfg5);
__host__ __device__ __forceinline__ void shape_w5(Geo& g) {
#define EEG_SET_(f) g.f = kGeoW5.f;
    EEG_FIELDS_W5(EEG_SET_)
#undef EEG_SET_
}

// Every field of GeoI (eegnet_infer_bf16.hip) that follows from the (validated) model dims: all but B, eps
// and the debug pointer.  PFU and lds are checked against their limits by make_geo_bf16.
constexpr GeoI geo_shape_bf16(ModelDims m) {
    GeoI g{};
    g.C = m.C; g.T = m.T; g.F1 = m.F1; g.D = m.D; g.K1 = m.K1;
    g.F2 = g.F1 * g.D;
    g.P = (g.K1 - 1) / 2;
    g.CP = rup(g.C, 32); g.KC = g.CP / 32;
    g.F2P = g.F2 <= 16 ? 16 : g.F2 <= 32 ? 32 : 64;
    g.NOT = g.F2P / 16;
    g.F2K = std::max(32, g.F2P); g.KCW = g.F2K / 32;
    g.TX = rup(g.T, 128);
    g.NT = (g.T + 15) / 16; g.NBLK = (g.NT + 15) / 16;
    g.LPs = g.P + 1;
    g.KSF = (g.K1 + 16 + 31) / 32;
    // s rows: FIR windows read up to element 256*NBLK + 32*KSF - 16; row stride = 4 mod 8 dwords so the
    // 16 rows of one spatial-tile store land on distinct bank quads
    g.SXs = 256 * g.NBLK + 32 * g.KSF - 8;
    g.T1 = g.T / 4; g.T2 = g.T1 / 8; g.NF = g.F2 * g.T2;
    param_offsets(g);
    const int nq = (g.T1 + 3) / 4;
    g.RA = 4 * nq + 16;
    g.NT1 = (8 * g.T2 + 15) / 16;
    g.TZ = rup(std::max(4 * nq, 16 * g.NT1), 128);
    if (g.T % 8 == 0) {
        const int u = (g.CP * g.TX / 8 + NTI - 1) / NTI;
        g.PFU = 1;
        while (g.PFU < u) g.PFU *= 2;
    }
    const int r1 = std::max(g.CP * g.TX * 2, rup(g.F2P * g.RA * 4, 16) + g.F2K * g.TZ * 2);
    g.offZ = rup(g.F2P * g.RA * 4, 16);
    g.offS = rup(r1, 16);
    g.offW1 = rup(g.offS + g.F2P * g.SXs * 2, 16);
    g.offW2 = rup(g.offW1 + g.F1 * g.K1 * 4, 16);
    g.offCo = rup(g.offW2 + g.F2P * K2 * 4, 16);
    g.offL = rup(g.offCo + 4 * g.F2P * 4, 16);
    g.lds = g.offL + NWI * NCLS * 4;
    // classifier weights staged in LDS when they fit (cfg5: 16 KB), else read from global
    const int offF = rup(g.lds, 16);
    if (offF + NCLS * g.NF * 4 <= LDS_MAX) {
        g.offF = offF;
        g.lds = offF + NCLS * g.NF * 4;
    }
    return g;
}

// k_infer_bf16_cfg5 hard-codes its dims (namespace c5) and takes the parameter offsets from the run-time
// GeoI; the host launches it for exactly the cfg5 dims (is_cfg5)
constexpr GeoI kGeoCfg5 = geo_shape_bf16(kDimsCfg5);
static_assert(c5::C == kGeoCfg5.C && c5::T == kGeoCfg5.T && c5::F1 == kGeoCfg5.F1 && c5::D == kGeoCfg5.D &&
              c5::F2 == kGeoCfg5.F2 && c5::K1 == kGeoCfg5.K1 && c5::T1 == kGeoCfg5.T1 && c5::T2 == kGeoCfg5.T2 &&
              c5::NF == kGeoCfg5.NF, "namespace c5 (eegnet_infer_bf16c.hip) is not the cfg5 geometry");

}  // namespace eeg
