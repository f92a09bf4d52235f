// eepacc_ab_impl.inc -- device code of the ABMPC kernels.  Included by eepacc_kernels.hip once per entry of its
// EEPACC_AB_VARIANTS list, each time into its own namespace EEPACC_IMPL_NS with the six switches EEPACC_IMPL_MB (move
// blocking compiled out / in), EEPACC_IMPL_BL (the baseline controller's row grouping, CreateQP_BL.m: one slack for all
// soft rows), EEPACC_IMPL_TV (with _BL: the target-vehicle MPC, CreateQP_TV.m: the baseline QP without its
// vehicle-following rows and without lead inputs), EEPACC_IMPL_ICE (the ICE-map fuel term, whose Hessian is built and
// inverted every step), EEPACC_IMPL_CLS (settings classes: every instance has the DevCfg of its class) and EEPACC_IMPL_EST
// (horizon guesses from the caller instead of the estimators: eepacc_ab_step_est, eepacc_run_abmpc_preview; with
// EEPACC_IMPL_CLS: eepacc_classes_step_est, eepacc_run_classes_preview), so that the default path carries no register or
// instruction cost for the variants.
// The tables of the active-set method (the inverse He of the effective Hessian, the inverse Schur block P of the working
// set) are maintained by eepacc_schur.h, and the steps of a dual pass that do not depend on the row catalogue are in
// eepacc_dual_step.h; the FBMPC kernels share both, and both are included once, outside these namespaces.
namespace eepacc {
namespace EEPACC_IMPL_NS {
using namespace wv;

constexpr bool kMoveBlocking = EEPACC_IMPL_MB;
constexpr bool kBaseline = EEPACC_IMPL_BL;
constexpr bool kIce = EEPACC_IMPL_ICE;      // ICE-map fuel term (CreateQP_AB.m:154-159): the Hessian changes every step
constexpr bool kTargetVeh = EEPACC_IMPL_TV;     // RunOpt_TVMPC (CreateQP_TV.m): a baseline variant (kBaseline is set too)
static_assert(!kTargetVeh || kBaseline, "the target-vehicle MPC is a variant of the baseline controller");
constexpr bool kClasses = EEPACC_IMPL_CLS;  // a handle of eepacc_create_classes / _classes_bl: the kernels' Cp is its array DevCfg[n_classes]
static_assert(!kClasses || !(kMoveBlocking || kIce), "settings classes are built for the plain ABMPC kernels and the two baseline variants only");
constexpr bool kEst = EEPACC_IMPL_EST;      // the kernels take horizon guesses as further arguments (DESIGN.md section 3.4f)
static_assert(!kEst || !(kMoveBlocking || kTargetVeh || kIce), "supplied horizon guesses are built for the plain ABMPC kernels and the baseline controller, with one DevCfg (est, blest) or with settings classes (clsest, blclsest), only");


#undef PTIC
#undef PTOC
#undef RTOC
#ifdef EEPACC_AB_TIMING
__device__ unsigned long long g_ab_prof[24];
#define PTIC(L) long long _pt = wall_clock64()
#define PTOC(L, slot) do { long long _n = wall_clock64(); (L).prof[slot] += _n - _pt; _pt = _n; } while (0)
#else
#define PTIC(L)
#define PTOC(L, slot)
#endif

constexpr double kInf = 1e300;
constexpr double kTolViol = 1e-11;
#ifdef EEPACC_BL_TRACE
__device__ int g_trace_on = 0;       // event trace of single-instance launches (tools/gpu_bl_trace*.py, tools/gpu_ab_trace_one.py)
#endif
constexpr double kTolDual = 1e-12;
constexpr int kSinglePasses = 14;
constexpr int kPfAdds = 4;        // rows a warm start may take in (primal first) before its negative multipliers are repaired
constexpr int kChunkStepsDefault = 16;      // MPC steps per work unit of the closed-loop kernel

// ----------------------------------------------------------------------------------------------
// row catalogue
__device__ __forceinline__ int group_of(int t) {
    // CreateQP_BL.m:232-312: every soft row of the baseline QP carries the one slack xi_f (R_VINC, R_HWP do not exist)
    if constexpr (kBaseline) return t < R_AMAX ? G_NONE : G_F;
    return t < R_AMAX ? G_NONE : (t < R_SAFE1 ? G_F : (t < R_VINC ? G_S : (t == R_VINC ? G_V : G_H)));
}
// Row types this variant has.  CreateQP_TV.m:229-284 is CreateQP_BL.m's stage without the two headway rows (and without
// the two rows of the terminal stage); the travel-incentive and headway-policy rows are ABMPC's alone.  The type
// numbering, and with it the nibble of a type in the state-code word, stays: the unrolled loops over the types skip the
// four at compile time, so 12 of the 16 nibbles and 12 of the 16 right-hand sides Lane::ba are live in this variant.
__device__ __forceinline__ constexpr bool row_live(int t) {
    return !kTargetVeh || !(t == R_SAFE1 || t == R_SAFE2 || t == R_VINC || t == R_HWP);
}
// the quadratic slack of the headway-policy row is above its bound at this lane (never, where the row type is compiled out)
#define EEPACC_HWP_ON(L) (row_live(R_HWP) && code_of(L, R_HWP) == 3)
__device__ __forceinline__ double row_al(int t) {
    return (t == R_SLO) ? -1.0 : ((t == R_SHI || t == R_SAFE1 || t == R_SAFE2 || t == R_HWP) ? 1.0 : 0.0);
}
__device__ __forceinline__ double row_be(int t, double tau_min, double chw) {
    switch (t) {
        case R_VLO: case R_VINC: return -1.0;
        case R_VHI: case R_VLIM: case R_VCURV: case R_VSTOP: case R_VTL: return 1.0;
        case R_SAFE2: return tau_min;
        case R_HWP: return chw;
        default: return 0.0;
    }
}
__device__ __forceinline__ double row_ga(int t) {
    return (t == R_AMAX || t == R_JMAX) ? 1.0 : ((t == R_AMIN || t == R_JMIN) ? -1.0 : 0.0);
}
__device__ __forceinline__ double row_de(int t, int k) {
    if (k == 0) return 0.0;
    return t == R_JMAX ? -1.0 : (t == R_JMIN ? 1.0 : 0.0);
}

template <int MMAX, int NS>
struct WaveMem {                 // one per wave, in LDS (followed by the wave's NS x NS matrix He)
    double P[MMAX * (MMAX + 1) / 2];
    double yv[NS], av[NS];
    double shv[NS + 1], vhv[NS + 1];
    double ub[NS + 1], sub[NS + 1], vub[NS + 1];     // images of a vector; also scratch of adjoint()
    double ws[NS + 1], wv[NS + 1], wa[NS + 1];
    double e_al[MMAX], e_be[MMAX], e_ga[MMAX], e_de[MMAX], e_d[MMAX];
    double lam[MMAX], sv[MMAX], rv[MMAX];
    // (the pivot column of the factor updates lives in ws | wv | wa, which are free while the factor is rebuilt)
    int w_k[MMAX];
};

// per-lane (= per-stage) registers of the wave's QP
struct Lane {
    int lane, N;
    double T, tau, tau1;          // T_k, tau_k, tau_{k+1}
    double tau_rev;               // tau_{N-lane} (reversed stage order, see adjoint())
    double ba[kNumRowTypes];      // a-space right-hand sides
    unsigned valid;               // bit t: row (t, lane) exists with a non-zero normal
#ifdef EEPACC_AB_TIMING
    long long prof[24];
#endif
    unsigned ign;                 // bit t / 16+g: duplicate row ignored during this solve
    unsigned long long kmask;     // wave-uniform: stages whose penalty q n n' is folded into He
    double lbF, lbS, lbV, lbH;    // slack lower bounds (constant rows of stage 0 fold in here)
    unsigned long long code;      // 4 bits per type: 0 off, 1 in working set, 2 group pivot, 3 compliant
    double chw;                   // headway-policy coefficient T_hwp + G_hwp*v_est(k)
    double g0;                    // base gradient of the condensed objective
    double a, sh, vh, am1;        // acceleration and homogeneous trajectories, a_{k-1}
    int base;                     // first working-set position of this lane's rows
};

__device__ __forceinline__ int code_of(const Lane& L, int t) { return (int)((L.code >> (4 * t)) & 15ull); }
__device__ __forceinline__ void set_code(Lane& L, int t, int c) {
    L.code = (L.code & ~(15ull << (4 * t))) | ((unsigned long long)c << (4 * t));
}

struct Cfg {   // wave-uniform scalars pulled out of DevCfg once
    int N;
    double tau_min, wF, wS, wV, wH, qH;
    int mb_len;                   // 0: no move blocking; else the longest block
    const int32_t *mb_lead, *mb_end;
};

// Move blocking (a_k = a_{k-1} where Mb[k] = 1, CreateQP_AB.m:282-288) as a change of variables
// a = E abar: every product with the inverse Hessian becomes E (E'HE)^-1 E'.  mb_reduce is E'
// (a block leader collects the covector entries of its block), mb_expand is E.
__device__ __forceinline__ double mb_reduce(const Lane& L, const Cfg& c, double x) {
    if constexpr (!kMoveBlocking) return x;
    if (c.mb_len == 0) return x;
    const int k = L.lane <= L.N ? L.lane : L.N;
    const int end = c.mb_end[k];
    const bool leader = c.mb_lead[k] == k && L.lane < L.N;
    double acc = x;
    for (int d = 1; d < c.mb_len; ++d) {
        const double y = __shfl_down(x, d, 64);
        if (L.lane + d <= end) acc += y;
    }
    return leader ? acc : 0.0;
}
__device__ __forceinline__ double mb_expand(const Lane& L, const Cfg& c, double x) {
    if constexpr (!kMoveBlocking) return x;
    if (c.mb_len == 0) return x;
    const int k = L.lane < L.N ? L.lane : 0;
    const double y = __shfl(x, c.mb_lead[k], 64);
    return L.lane < L.N ? y : x;
}

// the same two maps for a wave whose halves each carry a horizon of their own (eepacc_ab_cols.h): stage k = l & 31
__device__ __forceinline__ double mb_reduce_half(const Lane& L, const Cfg& c, double x) {
    if constexpr (!kMoveBlocking) return x;
    if (c.mb_len == 0) return x;
    const int hl = L.lane & 31;
    const int k = hl <= L.N ? hl : L.N;
    const int end = c.mb_end[k];
    const bool leader = c.mb_lead[k] == k && hl < L.N;
    double acc = x;
    for (int d = 1; d < c.mb_len; ++d) {
        const double y = __shfl_down(x, d, 64);
        if (hl + d <= end) acc += y;
    }
    return leader ? acc : 0.0;
}
__device__ __forceinline__ double mb_expand_half(const Lane& L, const Cfg& c, double x) {
    if constexpr (!kMoveBlocking) return x;
    if (c.mb_len == 0) return x;
    const int hl = L.lane & 31;
    const int k = hl < L.N ? hl : 0;
    const double y = __shfl(x, c.mb_lead[k] + (L.lane & 32), 64);
    return hl < L.N ? y : x;
}

__device__ __forceinline__ double group_w(const Cfg& c, int g) {
    return g == G_F ? c.wF : (g == G_S ? c.wS : (g == G_V ? c.wV : c.wH));
}
__device__ __forceinline__ double group_lb(const Lane& L, int g) {
    return g == G_F ? L.lbF : (g == G_S ? L.lbS : (g == G_V ? L.lbV : L.lbH));
}
__device__ __forceinline__ int lane_group(const Lane& L, int t) { return L.lane == L.N ? G_NONE : group_of(t); }

// value of row t at this lane for the current homogeneous trajectory (without slack)
__device__ __forceinline__ double row_val(const Lane& L, const Cfg& c, int t, double ba_t) {
    return row_al(t) * L.sh + row_be(t, c.tau_min, L.chw) * L.vh + row_ga(t) * L.a + row_de(t, L.lane) * L.am1 - ba_t;
}

// bit tricks on the 4-bit state codes (values 0..3: the upper two bits of every nibble are zero): bit 4t of the result
// is set where type t has the given code
constexpr unsigned long long kNib = 0x1111111111111111ull;
__device__ __forceinline__ unsigned long long codes_eq1(unsigned long long c) { return c & ~(c >> 1) & kNib; }
__device__ __forceinline__ unsigned long long codes_eq2(unsigned long long c) { return (c >> 1) & ~c & kNib; }
__device__ __forceinline__ constexpr unsigned long long type_range(int t0, int t1) {      // bit 4t of types t0..t1
    return ((t1 >= 15 ? ~0ull : ((1ull << (4 * (t1 + 1))) - 1ull)) & ~((1ull << (4 * t0)) - 1ull)) & kNib;
}
// number of this lane's working-set rows (code 1) of the types below t
__device__ __forceinline__ int rows_below(const Lane& L, int t) {
    return __popcll(codes_eq1(L.code) & ((1ull << (4 * t)) - 1ull));
}
// pivot type of linear group g at this lane (-1 if the group is in Z state)
__device__ __forceinline__ int pivot_of(const Lane& L, int g) {
    const unsigned long long rng = kBaseline ? (g == G_F ? type_range(R_AMAX, R_VINC) : 0ull)
                                             : (g == G_F ? type_range(R_AMAX, R_VCURV)
                                                         : (g == G_S ? type_range(R_SAFE1, R_VTL) : (g == G_V ? type_range(R_VINC, R_VINC) : 0ull)));
    const unsigned long long two = codes_eq2(L.code) & rng;
    return two ? ((__ffsll((long long)two) - 1) >> 2) : -1;
}

// homogeneous double-integrator response to the per-lane input x (lane k < N holds x_k):
//   vh_k = sum_{i<k} T_i x_i ,  sh_k = sum_{i<k} (T_i vh_i + T_i^2/2 x_i)
__device__ __forceinline__ void hom_traj(const Lane& L, double x, double& sh, double& vh) {
    double xi = (L.lane < L.N) ? x : 0.0;
    vh = scan_excl(L.T * xi);
    double inc = (L.lane < L.N) ? (L.T * vh + 0.5 * L.T * L.T * xi) : 0.0;
    sh = scan_excl(inc);
}

// Storage of the per-wave inverse He (layouts and products: eepacc_schur.h).  NS <= 32: full NS x NS (zero padded).
// NS = 64: packed lower triangle: 16.6 KB instead of 32 KB, which is what lets a third wave onto a CU at N = 60.
template <int NS> constexpr bool kPackedHe = NS > 32;
template <int NS> constexpr int kHeDoubles = kPackedHe<NS> ? NS * (NS + 1) / 2 : NS * NS;

// out = He yv for the passes of the solve: at NS = 32 the sum of a column is split over the two halves of the wave
template <int NS>
__device__ __forceinline__ double he_apply(const double* Hs, const double* yv, int N, int lane) {
    if constexpr (kPackedHe<NS>) return he_mul<NS, true>(Hs, yv, N, lane);
    else return he_mul_halves<NS>(Hs, yv, N, lane);
}

// a-space normal of the row (kq; al,be,ga,de) evaluated at this lane j:
__device__ __forceinline__ double normal_at(const Lane& L, int kq, double al, double be, double ga, double de, double tau_kq) {
    double c = 0.0;
    const int j = L.lane;
    if (j < L.N) {
        if (j < kq) c = L.T * (be + al * (0.5 * L.T + tau_kq - L.tau1));
        if (j == kq) c += ga;
        if (j == kq - 1) c += de;
    }
    return c;
}

// adjoint of the condensing: given stage weights on (s_k, v_k, a_k) in LDS (ws, wv, wa, k = 0..N)
// returns d/da_j of sum_k ws_k s_k + wv_k v_k + wa_k a_k  for lane j < N
template <int NS>
__device__ __forceinline__ double adjoint(const Lane& L, const double* ws, const double* wv, const double* wa, double* tmp) {
    // suffix sums over stages k > j are prefix sums over the reversed stage order: lane r holds
    // stage N - r; the three running sums are written back in stage order through LDS (wa[65..])
    const int r = L.lane, N = L.N;
    const int k = N - r;
    const bool in = k >= 0;
    const double s = in ? ws[k] : 0.0, v = in ? wv[k] : 0.0;
    const double tk = in ? L.tau_rev : 0.0;
    const double WS = scan_excl(s), WV = scan_excl(v), WST = scan_excl(s * tk);
    if (in) { tmp[k] = WS; tmp[(NS + 1) + k] = WV; tmp[2 * (NS + 1) + k] = WST; }
    WSYNC();
    const int j = L.lane;
    double g = 0.0;
    if (j < N) g = wa[j] + L.T * (tmp[(NS + 1) + j] + tmp[2 * (NS + 1) + j] - (L.tau1 - 0.5 * L.T) * tmp[j]);
    WSYNC();
    return g;
}

// The quadratic slack xi_h of stage k, once above its bound, is eliminated into the objective:
// H_eff = H + q * sum_k n_k n_k'  (n_k: a-space normal of the headway-policy row).  He holds
// H_eff^-1 for this wave; adding / removing one stage is a Sherman-Morrison rank-one update.
template <int MMAX, int NS>
__device__ __forceinline__ void he_rank1(const Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, double* He,
                                         const double* tauv, int k, bool add) {
    const int lane = L.lane, N = L.N;
    const double chwk = bcast(L.chw, k);
    const double nk = mb_reduce(L, c, normal_at(L, k, 1.0, chwk, 0.0, 0.0, tauv[k]));
    if (lane < NS) M.yv[lane] = nk;
    WSYNC();
    const double y = he_apply<NS>(He, M.yv, N, lane);          // in the reduced variables: the table is updated with it
    double sy, vy;
    hom_traj(L, mb_expand(L, c, y), sy, vy);
    const double ny = bcast(sy + chwk * vy, k);                 // n_k' y
    const double kappa = add ? c.qH / (1.0 + c.qH * ny) : -c.qH / (1.0 - c.qH * ny);
    if (lane < NS) M.ub[lane] = y;          // y is zero beyond N
    WSYNC();
    if constexpr (kPackedHe<NS>) {
        if (lane < NS) he_sub_outer<NS, true>(He, M.ub, kappa * y, lane);
    } else {
        he_sub_outer_halves<NS>(He, M.ub, kappa * M.ub[lane & (NS - 1)], lane);      // two lanes per column
    }
    WSYNC();
}

template <int MMAX, int NS>
__device__ __forceinline__ void he_sync(Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, double* He, const double* tauv) {
    if constexpr (!row_live(R_HWP)) return;
    const unsigned long long want = __ballot(L.lane < L.N && code_of(L, R_HWP) == 3);
    unsigned long long diff = want ^ L.kmask;
    while (diff) {
        const int k = __ffsll((long long)diff) - 1;
        diff &= diff - 1;
        he_rank1(L, c, M, He, tauv, k, ((want >> k) & 1ull) != 0ull);
    }
    L.kmask = want;
}

template <int NS>
__device__ __forceinline__ void he_load_base(double* He, const double* __restrict__ base, int N, int lane) {
    if constexpr (kPackedHe<NS>) {
        // lane j fills column j of the lower triangle (base is symmetric)
        if (lane < NS)
            for (int i = lane; i < NS; ++i) He[he_tri(i) + lane] = (i < N && lane < N) ? base[i * N + lane] : 0.0;
    } else {
#pragma unroll 4
        for (int e = lane; e < NS * NS; e += 64) {
            const int i = e / NS, j = e % NS;
            He[e] = (i < N && j < N) ? base[i * N + j] : 0.0;
        }
    }
}

// ----------------------------------------------------------------------------------------------
// rebuild the working-set list + effective rows from the state codes, build S = C Hinv C' + D,
// invert it in place.  returns m (or -1 if S was numerically singular).  F says which of the three ways of
// eepacc_schur.h brings P up to date: bordered update, downdate or full rebuild.
template <int MMAX, int NS>
__device__ __forceinline__ int rebuild_and_factor(Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, double* Hs, const double* tauv,
                                                  const FastInfo& F) {
    const int lane = L.lane, N = L.N;
#undef RTOC
#ifdef EEPACC_AB_TIMING
    long long _q = wall_clock64();
#define RTOC(slot) do { long long _n = wall_clock64(); L.prof[slot] += _n - _q; _q = _n; } while (0)
#else
#define RTOC(slot)
#endif
    he_sync(L, c, M, Hs, tauv);
    RTOC(9);
    // count this lane's active rows
    const int cnt = __popcll(codes_eq1(L.code));
    double basef = scan_excl((double)cnt);
    L.base = (int)(basef + 0.5);
    int m = (int)(wave_sum((double)cnt) + 0.5);
    if (m > schur_capacity<MMAX>()) return -2;      // one row per lane (eepacc_schur.h): at most 64, whatever the tables hold
    // the pivot row of each linear group at this lane (what an active member is measured against), once per call
    struct PRow { double al, be, ga, de, d; };
    PRow PR[3];
#pragma unroll
    for (int gi = 0; gi < 3; ++gi) {
        const int g = G_F + gi;
        const int p = pivot_of(L, g);
        PRow r{0.0, 0.0, 0.0, 0.0, -group_lb(L, g)};
        if (p >= 0) {
            double pba = 0.0;
#pragma unroll
            for (int u = R_AMAX; u <= R_VINC; ++u) if (row_live(u) && u == p) pba = L.ba[u];
            r.al = row_al(p); r.be = row_be(p, c.tau_min, L.chw); r.ga = row_ga(p); r.de = row_de(p, lane); r.d = pba;
        }
        PR[gi] = r;
    }
    int pos = L.base;
#pragma unroll
    for (int t = 0; t < kNumRowTypes; ++t) {
        if (!row_live(t)) continue;
        int cd = code_of(L, t);
        if (cd == 1) {
            int g = lane_group(L, t);
            double al = row_al(t), be = row_be(t, c.tau_min, L.chw), ga = row_ga(t), de = row_de(t, lane);
            double d = L.ba[t];
            if (g == G_H) {
                d += L.lbH;
            } else if (g != G_NONE) {
                const int gi = group_of(t) - G_F;          // compile-time after unrolling (g itself depends on the lane)
                if (gi >= 0 && gi < 3) { const PRow& r = PR[gi]; al -= r.al; be -= r.be; ga -= r.ga; de -= r.de; d -= r.d; }
            }
            M.e_al[pos] = al; M.e_be[pos] = be; M.e_ga[pos] = ga; M.e_de[pos] = de;
            M.e_d[pos] = d; M.w_k[pos] = lane;
            ++pos;
        }
    }
    WSYNC();
    RTOC(10);
    if (m == 0) return 0;
    const unsigned short* rc = rc_table<MMAX>();
    if (F.fast == 1 && m == F.m_old + 1 && F.m_old > 0) {
        // position of the new row in the new (lane-major) list
        const int pl = rows_below(L, F.tq);
        const int p = __builtin_amdgcn_readlane(L.base + pl, __builtin_amdgcn_readfirstlane(F.kq));
        schur_insert(M.P, M.rv, rc, m, p, 1.0 / F.zz, lane);
        RTOC(12);
        return m;
    }
    if (F.fast == 2 && m == F.m_old - 1) {
        schur_remove(M.P, M.ws, rc, F.m_old, m, F.drop_pos, lane);
        RTOC(12);
        return m;
    }
    // S columns: u_j = He c_j, two columns per pass: each He element is loaded once for both products,
    // the scan chains of the two trajectories overlap, and row i picks the images at its stage with
    // lane shuffles (no LDS round trip).  Input vectors in yv | lam (free while the factor is rebuilt).
    if constexpr (!kPackedHe<NS>) {
        // four columns per pass, two per half of the wave (eepacc_ab_cols.h); P is the two-column loop's bit for bit
        ab_schur_columns4<NS>(M, Hs, tauv, m, N, lane, half_lo(L.T), half_lo(L.tau1),
                              [&](double x) { return mb_reduce_half(L, c, x); }, [&](double x) { return mb_expand_half(L, c, x); });
    } else {
        const int ki = lane < m ? M.w_k[lane] : 0;
        const int kim1 = ki > 0 ? ki - 1 : 0;
        const double eal = lane < m ? M.e_al[lane] : 0.0, ebe = lane < m ? M.e_be[lane] : 0.0;
        const double ega = (lane < m && ki < N) ? M.e_ga[lane] : 0.0;
        const double ede = (lane < m && ki > 0 && ki <= N) ? M.e_de[lane] : 0.0;
        for (int j = 0; j < m; j += 2) {
            const bool two = j + 1 < m;
            const int j1 = two ? j + 1 : j;
            const int kj0 = M.w_k[j], kj1 = M.w_k[j1];
            const double c0 = mb_reduce(L, c, normal_at(L, kj0, M.e_al[j], M.e_be[j], M.e_ga[j], M.e_de[j], tauv[kj0]));
            const double c1 = mb_reduce(L, c, normal_at(L, kj1, M.e_al[j1], M.e_be[j1], M.e_ga[j1], M.e_de[j1], tauv[kj1]));
            if (lane < NS) { M.yv[lane] = c0; M.lam[lane] = c1; }
            WSYNC();
            double u0, u1;
            he_mul2<NS, kPackedHe<NS>>(Hs, M.yv, M.lam, N, lane, u0, u1);
            u0 = mb_expand(L, c, u0); u1 = mb_expand(L, c, u1);
            WSYNC();
            double su0, vu0, su1, vu1;
            hom_traj(L, u0, su0, vu0);
            hom_traj(L, u1, su1, vu1);
            const double sx = eal * __shfl(su0, ki, 64) + ebe * __shfl(vu0, ki, 64) + ega * __shfl(u0, ki, 64) + ede * __shfl(u0, kim1, 64);
            const double sy = eal * __shfl(su1, ki, 64) + ebe * __shfl(vu1, ki, 64) + ega * __shfl(u1, ki, 64) + ede * __shfl(u1, kim1, 64);
            if (lane >= j && lane < m) M.P[pidx(lane, j)] = sx;
            if (two && lane >= j + 1 && lane < m) M.P[pidx(lane, j + 1)] = sy;
        }
        WSYNC();
    }
    RTOC(11);
    // (scratch column in ws | wv | wa: 3 (NS + 1) >= MMAX doubles)
    const int singular = schur_invert(M.P, M.sv, M.ws, rc, m, lane);
    RTOC(12);
    if (singular) return kBaseline ? -(9 + singular) : -1;        // baseline controller: -(10 + list position of the dependent row)
    return m;
}

// gradient-side vector: g_eff + (incoming multiplier) * c_q + C' lam   evaluated per lane
template <int MMAX, int NS>
__device__ __forceinline__ double gradient_side(const Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, int m, bool with_lam,
                                double lam_q, int kq, double qal, double qbe, double qga, double qde) {
    const int lane = L.lane, N = L.N;
    // pivot rows act like working-set rows with multiplier w_g (own stage: plain stores)
    double s = 0.0, v = 0.0, a0 = 0.0, a1 = 0.0;   // a1 -> stage lane-1
    if (lane < N) {
#pragma unroll
        for (int t = R_AMAX; t <= R_VINC; ++t) {
            if (row_live(t) && code_of(L, t) == 2) {
                double w = group_w(c, group_of(t));
                s += w * row_al(t); v += w * row_be(t, c.tau_min, L.chw);
                a0 += w * row_ga(t); a1 += w * row_de(t, lane);
            }
        }
    }
    if (lane < N && EEPACC_HWP_ON(L)) {
        // quadratic slack above its bound: penalty w*xi + q/2 xi^2, xi = n'a - b; linear part (w - q b) n
        const double wl = c.wH - c.qH * L.ba[R_HWP];
        s += wl * row_al(R_HWP); v += wl * row_be(R_HWP, c.tau_min, L.chw);
    }
    if (lane <= N) { M.ws[lane] = s; M.wv[lane] = v; M.wa[lane] = a0; }
    WSYNC();
    if (lane > 0 && lane < N && a1 != 0.0) atomicAdd(&M.wa[lane - 1], a1);
    if (with_lam) scatter_rows(M, m, N, lane, M.lam, 1.0);
    if (lam_q != 0.0 && lane == 0) scatter_row(M, kq, N, lam_q, qal, qbe, qga, qde);
    WSYNC();
    double g = adjoint<NS>(L, M.ws, M.wv, M.wa, M.ub);
    return (lane < N) ? g + L.g0 : 0.0;
}

// a-space covector  c_q - C' r  of a step's primal direction (no objective part), per lane.  Uses ub/sub/vub as scratch.
template <int MMAX, int NS>
__device__ __forceinline__ double direction_side(const Lane& L, WaveMem<MMAX, NS>& M, int m, int kq,
                                                 double qal, double qbe, double qga, double qde) {
    const int lane = L.lane, N = L.N;
    if (lane <= N) { M.ws[lane] = 0.0; M.wv[lane] = 0.0; M.wa[lane] = 0.0; }
    WSYNC();
    scatter_rows(M, m, N, lane, M.rv, -1.0);
    if (lane == 0) scatter_row(M, kq, N, 1.0, qal, qbe, qga, qde);
    WSYNC();
    return adjoint<NS>(L, M.ws, M.wv, M.wa, M.ub);
}

// primal point from the multipliers: a = -Hinv (g_eff + lam_q c_q + C' lam); also refreshes the
// homogeneous trajectories and their LDS images (av/shv/vhv)
template <int MMAX, int NS>
__device__ __forceinline__ void primal_from_multipliers(Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, const double* Hs, int m,
                                        double lam_q, int kq, double qal, double qbe, double qga, double qde,
                                        double& grad_total) {
    double g = gradient_side(L, c, M, m, true, lam_q, kq, qal, qbe, qga, qde);
    grad_total = g;
    g = mb_reduce(L, c, g);
    if (L.lane < NS) M.yv[L.lane] = g;
    WSYNC();
    L.a = -mb_expand(L, c, he_apply<NS>(Hs, M.yv, L.N, L.lane));
    hom_traj(L, L.a, L.sh, L.vh);
    L.am1 = lane_prev(L.a);
    if (L.lane < L.N) M.av[L.lane] = L.a;
    if (L.lane <= L.N) { M.shv[L.lane] = L.sh; M.vhv[L.lane] = L.vh; }
    WSYNC();
}

// primal point + iterative refinement (refine_rounds, eepacc_dual_step.h); returns the relative residual of the
// working-set rows before any correction
template <int MMAX, int NS>
__device__ __forceinline__ double refine_primal(Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, const double* Hs, int m,
                                                double lam_q, int kq, double qal, double qbe, double qga, double qde,
                                                double& grad_total, int max_rounds, double res_tol) {
    return refine_rounds(M, m, L.N, L.lane, max_rounds, res_tol,
                         [&]() __attribute__((always_inline)) { primal_from_multipliers(L, c, M, Hs, m, lam_q, kq, qal, qbe, qga, qde, grad_total); });
}

// slack of linear group g at this lane for the current point
__device__ __forceinline__ double group_xi(const Lane& L, const Cfg& c, int g) {
    int p = pivot_of(L, g);
    if (p < 0) return group_lb(L, g);
    double pba = 0.0;
#pragma unroll
    for (int u = R_AMAX; u <= R_VINC; ++u) if (row_live(u) && u == p) pba = L.ba[u];
    return row_val(L, c, p, pba);
}

// ----------------------------------------------------------------------------------------------
// the dual active-set solve.  On entry L.code holds the (warm) working set; on exit the optimal
// one, L.a the accelerations, L.lamt the multipliers per (lane, type).
// repair of dual infeasibilities of a warm working set (multipliers in L.lamt).  The first passes
// fix only the worst one (a single wrong row usually drags many multipliers negative; dropping
// them all would throw the warm start away), later passes fix all of them at once.
template <int MMAX, int NS>
// returns 0: nothing to repair, 1: working set changed, 2: the only change is that the plain row at list
// position drop_pos left the working set (the factor can be downdated instead of rebuilt)
__device__ __forceinline__ int warm_repair(Lane& L, const Cfg& c, const WaveMem<MMAX, NS>& M, int m, bool single, int& drop_pos) {
    const int lane = L.lane, N = L.N;
    double lmax = 0.0;
    if (lane < m) lmax = fabs(M.lam[lane]);
    lmax = wave_max(lmax);
    const double tol = kTolDual * (1.0 + lmax);
    int changed = 0;
    double sumF = 0.0, sumS = 0.0, sumV = 0.0;
    double bestF = -1e300, bestS = -1e300, bestV = -1e300;     // largest multiplier per group
    int bF = -1, bS = -1, bV = -1;
    double worst = tol; int fix = EvCode::kNoEvent;
    int pos = L.base;
#pragma unroll
    for (int t = 0; t < kNumRowTypes; ++t) {
        if (!row_live(t)) continue;
        int cd = code_of(L, t);
        if (cd != 1) continue;
        int g2 = lane_group(L, t);
        double l = M.lam[pos++];
        if (g2 == G_H) {
            if (-l > tol) {
                if (!single) { set_code(L, t, 0); changed = 1; } else if (-l > worst) { worst = -l; fix = EvCode::pack(EV_DROP, lane, t); }
            } else if (l - c.wH > tol) {
                if (!single) { set_code(L, t, 3); changed = 1; } else if (l - c.wH > worst) { worst = l - c.wH; fix = EvCode::pack(EV_COMPL, lane, t); }
            }
        } else {
            if (-l > tol) {
                if (!single) { set_code(L, t, 0); changed = 1; l = 0.0; } else if (-l > worst) { worst = -l; fix = EvCode::pack(EV_DROP, lane, t); }
            } else if (g2 == G_F) { if (l > bestF) { bestF = l; bF = t; } }
            else if (g2 == G_S) { if (l > bestS) { bestS = l; bS = t; } }
            else if (g2 == G_V) { if (l > bestV) { bestV = l; bV = t; } }
            if (g2 == G_F) sumF += l; else if (g2 == G_S) sumS += l; else if (g2 == G_V) sumV += l;
        }
    }
    // group margins (bound multiplier in Z, pivot multiplier in P)
    int capg = 0;
    if (lane < N) {
#pragma unroll
        for (int g2 = G_F; g2 <= G_V; ++g2) {
            double sum = g2 == G_F ? sumF : (g2 == G_S ? sumS : sumV);
            double w = group_w(c, g2);
            double viol = sum - w;
            if (viol > tol * (1.0 + w)) {
                if (single) { if (viol > worst) { worst = viol; fix = EvCode::pack(EV_CAP, lane, g2); } }
                else if (!changed && !capg) capg = g2;
            }
        }
    }
    int el = -1, et = capg, plain_drop = 0;
    if (single) {
        wave_argmax(worst, fix);
#ifdef EEPACC_BL_TRACE
        if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("   repair: lmax %.3e worst %.3e fix(%d,%d,%d)\n", lmax, worst, fix >> 16, (fix >> 5) & 63, fix & 31);
#endif
        if (fix != EvCode::kNoEvent) {
            changed = 1;
            const int ek = EvCode::kind(fix);
            el = EvCode::lane(fix); et = EvCode::type(fix);
            if (ek == EV_DROP) {
                const int pl = rows_below(L, et);
                drop_pos = __builtin_amdgcn_readlane(L.base + pl, __builtin_amdgcn_readfirstlane(el));
                plain_drop = 1;
            }
            if (lane == el) {
                if (ek == EV_DROP) set_code(L, et, 0);
                else if (ek == EV_COMPL) set_code(L, et, 3);
            }
            if (ek != EV_CAP) el = -1;
        } else el = -1;
    } else if (capg) { el = lane; changed = 1; }
    if (lane == el) {          // group cap violated: make the member with the largest multiplier the pivot
        int p = pivot_of(L, et);
        if (p >= 0) set_code(L, p, 0);
        int bestt = et == G_F ? bF : (et == G_S ? bS : bV);
        if (bestt >= 0 && code_of(L, bestt) == 1) set_code(L, bestt, 2);
    }
    return __any(changed) ? (plain_drop ? 2 : 1) : 0;
}

// most violated inactive row / slack bound: returns lane*32 + code (code: row type, or 16+group for
// the bound of a slack) or -1; best = its scaled violation
// this lane's most violated row / slack bound: code (row type, or 16+group) or -1; myb = its scaled violation
__device__ __forceinline__ int lane_violation(const Lane& L, const Cfg& c, double tolv, double& myb_out) {
    const int lane = L.lane, N = L.N;
    double xiF = 0, xiS = 0, xiV = 0;
    if (lane < N) { xiF = group_xi(L, c, G_F); xiS = group_xi(L, c, G_S); xiV = group_xi(L, c, G_V); }
    // scaled violation val / (1 + |b|): candidates are compared cross-multiplied (one division per lane instead of one per
    // row type); bestv / bests is this lane's best so far, starting at the tolerance
    double bestv = tolv, bests = 1.0; int myp = -1;
    const unsigned cand = L.valid & ~L.ign;
#pragma unroll
    for (int t = 0; t < kNumRowTypes; ++t) {
        if (!row_live(t)) continue;
        if (!((cand >> t) & 1u)) continue;
        if (code_of(L, t) != 0) continue;
        int g2 = lane_group(L, t);
        double val = row_val(L, c, t, L.ba[t]);
        val -= (g2 == G_F) ? xiF : (g2 == G_S ? xiS : (g2 == G_V ? xiV : (g2 == G_H ? L.lbH : 0.0)));
        const double sc = 1.0 + fabs(L.ba[t]);
        if (val * bests > bestv * sc) { bestv = val; bests = sc; myp = t; }
    }
    double myb = bestv / bests;
    if (lane < N) {
        if (pivot_of(L, G_F) >= 0 && !((L.ign >> (16 + G_F)) & 1u) && L.lbF - xiF > myb) { myb = L.lbF - xiF; myp = 16 + G_F; }
        if (pivot_of(L, G_S) >= 0 && !((L.ign >> (16 + G_S)) & 1u) && L.lbS - xiS > myb) { myb = L.lbS - xiS; myp = 16 + G_S; }
        if (pivot_of(L, G_V) >= 0 && !((L.ign >> (16 + G_V)) & 1u) && L.lbV - xiV > myb) { myb = L.lbV - xiV; myp = 16 + G_V; }
        // penalised quadratic slack: xi_h = n'a - b must stay above its bound
        if (EEPACC_HWP_ON(L) && !((L.ign >> (16 + G_H)) & 1u)) {
            double xih = row_val(L, c, R_HWP, L.ba[R_HWP]);
            if (L.lbH - xih > myb) { myb = L.lbH - xih; myp = 16 + G_H; }
        }
    }
    myb_out = myb;
    return myp;
}
__device__ __forceinline__ int find_violation(const Lane& L, const Cfg& c, double tolv, double& best) {
    const int myp = lane_violation(L, c, tolv, best);
    int bp = (myp < 0) ? 0x7fffffff : (L.lane * 32 + myp);
    wave_argmax(best, bp);
    return bp == 0x7fffffff ? -1 : bp;
}

// Baseline controller (one slack group): the rows outside the working set are affine along the segment from the point L0 to
// the point L and beyond while the group states stay; returns the largest t >= 0 such that none of them is violated at
// L + t (L - L0)   (kInf: the ray stays feasible).
__device__ __forceinline__ double slide_limit(const Lane& L, const Lane& L0, const Cfg& c) {
    const int lane = L.lane, N = L.N;
    double xi1 = 0, xi0 = 0;
    if (lane < N) { xi1 = group_xi(L, c, G_F); xi0 = group_xi(L0, c, G_F); }
    double best = kInf;
    const unsigned cand = L.valid & ~L.ign;
#pragma unroll
    for (int t = 0; t < kNumRowTypes; ++t) {
        if (!row_live(t)) continue;
        if (!((cand >> t) & 1u)) continue;
        if (code_of(L, t) != 0) continue;
        const bool soft = lane_group(L, t) == G_F;
        const double v1 = row_val(L, c, t, L.ba[t]) - (soft ? xi1 : 0.0);
        const double v0 = row_val(L0, c, t, L.ba[t]) - (soft ? xi0 : 0.0);
        const double sl = v1 - v0;
        if (sl > 0.0) best = fmin(best, fmax(-v1, 0.0) / sl);
    }
    if (lane < N && pivot_of(L, G_F) >= 0 && !((L.ign >> (16 + G_F)) & 1u)) {
        const double v1 = L.lbF - xi1, sl = xi0 - xi1;
        if (sl > 0.0) best = fmin(best, fmax(-v1, 0.0) / sl);
    }
    int dummy = lane;
    wave_argmin(best, dummy);
    return best;
}

// right-hand side ba[t] of lane k for wave-uniform t and k: a scalar switch picks the register, one broadcast
__device__ __forceinline__ double ba_at(const Lane& L, int t, int k) {
    double x = 0.0;
    switch (t) {          // (types the variant does not have, row_live, fall through to the default)
        case 0: x = L.ba[0]; break;   case 1: x = L.ba[1]; break;   case 2: x = L.ba[2]; break;   case 3: x = L.ba[3]; break;
        case 4: x = L.ba[4]; break;   case 5: x = L.ba[5]; break;   case 6: x = L.ba[6]; break;   case 7: x = L.ba[7]; break;
        case 8: x = L.ba[8]; break;   case 9: x = L.ba[9]; break;
        case 10: if constexpr (row_live(10)) { x = L.ba[10]; break; }
        case 11: if constexpr (row_live(11)) { x = L.ba[11]; break; }
        case 12: x = L.ba[12]; break; case 13: x = L.ba[13]; break;
        case 14: if constexpr (row_live(14)) { x = L.ba[14]; break; }
        default: x = L.ba[row_live(15) ? 15 : 13]; break;
    }
    return bcast(x, k);
}

// effective a-space row of the incoming constraint for the current group states.  Everything that decides it is
// wave-uniform (its stage kq, its type, the pivot type of its group at lane kq), so the coefficients are scalar
// arithmetic and only the right-hand sides and the headway coefficient are fetched from lane kq.
__device__ __forceinline__ void incoming_row(const Lane& L, const Cfg& c, Incoming& q) {
    const int kq = q.kq;
    const double chw = bcast(L.chw, kq);
    double qal = 0, qbe = 0, qga = 0, qde = 0, qd = 0;
    if (!q.is_bound) {
        const int tq = q.tq;
        qal = row_al(tq); qbe = row_be(tq, c.tau_min, chw); qga = row_ga(tq); qde = row_de(tq, kq);
        qd = ba_at(L, tq, kq);
        if (q.gq == G_H) {
            qd += bcast(L.lbH, kq);
        } else if (q.gq != G_NONE) {
            const int p = __builtin_amdgcn_readlane(pivot_of(L, q.gq), __builtin_amdgcn_readfirstlane(kq));
            if (p >= 0) {
                qal -= row_al(p); qbe -= row_be(p, c.tau_min, chw); qga -= row_ga(p); qde -= row_de(p, kq);
                qd -= ba_at(L, p, kq);
            } else qd += bcast(group_lb(L, q.gq), kq);
        }
    } else if (q.gq == G_H) {
        qal = -row_al(R_HWP); qbe = -row_be(R_HWP, c.tau_min, chw);
        qd = -(ba_at(L, R_HWP, kq) + bcast(L.lbH, kq));
    } else {
        const int p = __builtin_amdgcn_readlane(pivot_of(L, q.gq), __builtin_amdgcn_readfirstlane(kq));
        qal = -row_al(p); qbe = -row_be(p, c.tau_min, chw); qga = -row_ga(p); qde = -row_de(p, kq);
        qd = -(ba_at(L, p, kq) + bcast(group_lb(L, q.gq), kq));
    }
    q.al = qal; q.be = qbe; q.ga = qga; q.de = qde; q.d = qd;
}

// ----------------------------------------------------------------------------------------------
// the dual active-set solve.  On entry L.code holds the (warm) working set; on exit the optimal
// one, L.a the accelerations, L.lamt the multipliers per (lane, type).  One loop, one working-set
// change per pass: [rebuild + factor] -> [multipliers] -> [primal + refinement] -> either repair the
// warm start, or pick the next violated constraint / continue the current one and take the step.
template <int MMAX, int NS>
__device__ __forceinline__ SolveStats solve_qp(Lane& L, const Cfg& c, WaveMem<MMAX, NS>& M, double* Hs, const double* Hbase,
                               const double* tauv, int max_iter, double& grad_total) {
    const int lane = L.lane, N = L.N;
    SolveStats st{0, 0, 0, 0};
    int m = 0;
    bool warm = true, have_q = false;
    int pass = 0;
    double lam_q = 0.0, best = 0.0;
    Incoming q{0, 0, 0, 0, false, 0, 0, 0, 0, 0};
    FastInfo F{0, 0, 0, 0, 0, 1.0};   // what the last event did to the working set (see rebuild_and_factor)
    int fast_run = 0;
    bool p_stale = false;     // the updated inverse no longer solves its system to working accuracy
    bool inc_next = false;    // the point and the multipliers have been carried along the last step
    bool carry_ok = true;     // cleared for the rest of the solve once a carried point missed its rows (huge multipliers of an infeasible QP)
    bool pf = false;          // the incoming row was taken while the warm set still has (moderately) negative multipliers
    int pf_left = kPfAdds;
    int dep_drops = 0;        // baseline controller: dependent rows taken out of a warm working set
    double tol_floor = 0.0;   // baseline controller: violation tolerance lifted over the measured resolution of a degenerate vertex
    constexpr int kHist = 8;  // longest recurrence looked for (measured: periods 2 and 7)
    int hist_bp[kHist];
    double hist_best[kHist];
#pragma unroll
    for (int h = 0; h < kHist; ++h) { hist_bp[h] = -1; hist_best[h] = 0.0; }
#ifdef EEPACC_AB_TIMING
    int why = 0;
#define WHY(x) why = (x)
#else
#define WHY(x)
#endif
    for (;;) {
        PTIC(L);
#ifdef EEPACC_AB_TIMING
        L.prof[13] += 1; if (F.fast == 1) L.prof[3] += 1000000; if (F.fast == 2) L.prof[4] += 1000000;
#endif
        // the incremental updates are exact in exact arithmetic; rounding accumulates, so the factor is
        // rebuilt after six updates in a row (with the ORIG weights, 1e2 .. 1e7, longer runs cost
        // digits), or earlier if the multipliers it yields miss the working-set rows by more than 1e-10
        if (F.fast != 0 && (++fast_run > 6 || p_stale)) { F.fast = 0; WHY(6); }
        p_stale = false;
#ifdef EEPACC_AB_TIMING
        if (F.fast == 0) L.prof[14 + why] += 1;
#endif
        if (F.fast == 0) fast_run = 0;
        // the last pass ended with a plain row entering or leaving and already moved the primal point and the
        // multipliers along the step (below): nothing to recompute unless the factor is rebuilt anyway
        const bool inc = inc_next && F.fast != 0;
        inc_next = false;
        F.m_old = m;
        m = rebuild_and_factor(L, c, M, Hs, tauv, F);
        F.fast = 0;
        PTOC(L, 0);
        if constexpr (kBaseline) {
            // A shifted LP vertex (as many rows as variables) is often linearly dependent by one or two rows: the row at which the
            // factorisation broke down leaves the working set and the rest is tried again, before everything is thrown away
            // (measured on launches from rest: every step failed here and was solved from the empty set, 200 events each).
            if (m <= -10 && warm && dep_drops < 8) {
                const int p = -m - 10;
                const int pl = M.w_k[p];
                if (lane == pl) {
                    int idx = p - L.base;
#pragma unroll
                    for (int t = 0; t < kNumRowTypes; ++t) if (row_live(t) && code_of(L, t) == 1) { if (idx == 0) set_code(L, t, 0); --idx; }
                }
                ++dep_drops;
                WSYNC();
                continue;
            }
        }
        if (m < 0) {
#ifdef EEPACC_BL_TRACE
            if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("   factor failed (m %d, warm %d)\n", m, (int)warm);
#endif
            if (!warm) { st.status = 2; break; }
            L.code = 0ull;                 // unusable warm start: cold start
            he_load_base<NS>(Hs, Hbase, N, lane);
            L.kmask = 0ull;
            WSYNC();
            warm = false;
            continue;
        }
        if (have_q) incoming_row(L, c, q);
        bool scratch = !inc;
        double rel0 = 0.0;
        if (inc && m > 0) {
            // the carried point must satisfy the working-set rows; if not (stale factor, cancellation) fall back
            double rel = 0.0;
            if (lane < m) rel = fabs(rows_dot_img(M, lane, N, M.av, M.shv, M.vhv) - M.e_d[lane]) / (1.0 + fabs(M.e_d[lane]));
            int dummy = lane;
            wave_argmax(rel, dummy);
            rel0 = rel;
            if (rel0 > 1e-11) { scratch = true; carry_ok = false; }
#ifdef EEPACC_AB_TIMING
            L.prof[23] += scratch ? 1000 : 1;
#endif
        }
        if (scratch && m > 0) {
            // multipliers of the working set for the current incoming multiplier
            double g = mb_reduce(L, c, gradient_side(L, c, M, 0, false, lam_q, q.kq, q.al, q.be, q.ga, q.de));
            if (lane < NS) M.yv[lane] = g;
            WSYNC();
            double h = mb_expand(L, c, he_apply<NS>(Hs, M.yv, N, lane));
            double shh, vhh;
            hom_traj(L, h, shh, vhh);
            if (lane < N) M.ub[lane] = h;
            if (lane <= N) { M.sub[lane] = shh; M.vub[lane] = vhh; }
            WSYNC();
            solve_multipliers(M, m, lane, N);
        }
        PTOC(L, 1);
        // working accuracy while the working set is still changing; polished after convergence
        if (scratch) {
            const double r0 = refine_primal(L, c, M, Hs, m, lam_q, q.kq, q.al, q.be, q.ga, q.de, grad_total, 3, 1e-11);
            if (r0 > rel0) rel0 = r0;
        }
        if (fast_run > 0 && rel0 > 1e-10) p_stale = true;
        PTOC(L, 2);
        if (warm && !have_q) {
            if (m > 0) {
                // Primal first.  A shifted working set that rides a constraint over an interval of stages (headway policy behind a
                // slowing lead) is right in its middle and wrong at its ends; the middle rows' multipliers then come out moderately
                // negative, the repair below takes them out one pass at a time and the iteration puts them back one pass at a time.
                // While the negative multipliers are moderate, the most violated plain row goes through the ordinary step of the
                // iteration FIRST (its fast factor update included); rows with a negative multiplier cannot block that step (they
                // are treated as equalities for its duration).  When nothing is violated any more, what is still negative is repaired.
                bool take = false;
                if constexpr (kPfAdds > 0 && !kBaseline) {
                    if (pf_left > 0) {
                        const double lam_l = (lane < m) ? M.lam[lane] : 0.0;
                        const double labs = wave_max(fabs(lam_l)), lneg = wave_max(-lam_l);
                        if (lneg > kTolDual * (1.0 + labs) && lneg <= 0.3 * labs) {
                            const int bpw = find_violation(L, c, 1e-6, best);
                            if (bpw >= 0 && (bpw & 31) < 16) {
                                q.kq = bpw >> 5; q.qcode = bpw & 31; q.is_bound = false; q.tq = q.qcode;
                                q.gq = (q.kq == N) ? G_NONE : group_of(q.qcode);
                                have_q = true; lam_q = 0.0; pf = true; take = true;
                                --pf_left; ++st.iters;
                                incoming_row(L, c, q);
#ifdef EEPACC_BL_TRACE
                                if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("   primal first: (%d,%d) viol %.3e, worst multiplier %.3e of %.3e, m %d\n", q.kq, q.qcode, best, -lneg, labs, m);
#endif
                            }
                        }
                    }
                }
                if (!take) {
                const int rep = warm_repair(L, c, M, m, pass < kSinglePasses, F.drop_pos);
#ifdef EEPACC_BL_TRACE
                if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("   repair pass %d: m %d -> change %d\n", pass, m, rep);
#endif
                PTOC(L, 3);
                if (rep == 2) F.fast = 2;
                WHY(1);
                if (rep) {
                    if (++pass >= kSinglePasses + 6) {
                        // the repair does not settle: every plain row leaves the working set, the states of the slack groups
                        // stay (a group in P state has its pivot's multiplier w - 0 >= 0 and a penalised headway row has
                        // w_h + q xi_h: the set is dual feasible by construction; a state that is wrong shows up as a violated
                        // slack bound in the iteration).  An empty start would first walk every stage's travel-incentive
                        // slack off its bound again, one iteration per stage (measured: 29 of the 42 iterations of such a step).
                        L.code &= ~codes_eq1(L.code);
                        he_load_base<NS>(Hs, Hbase, N, lane);
                        L.kmask = 0ull;
                        WSYNC();
                        warm = false;
                    }
                    continue;
                }
                }
            }
            if (!have_q) warm = false;
        }
        if (!have_q) {
            const double tolv = viol_tolerance(kTolViol, st.iters, N);      // at most 1000 kTolViol = 1e-8, scaled by 1 + |b|
            int bp = find_violation(L, c, tolv > tol_floor ? tolv : tol_floor, best);
            if constexpr (kBaseline) {
                // Resolution of a degenerate LP vertex.  At a standstill every later stage's rows are dependent and the
                // multipliers reach w_f = 1e7 against the curvature bl_eps: the row values are only defined to 1e-5 .. 1e-3,
                // and two slack bounds violated by less than that can keep exchanging their stages' states for ever (measured:
                // use case 10, and 0.5 % of the braking starts of the S2 scenarios).  A violation that comes back with the same
                // value after the working set has been through the same states is below what the arithmetic resolves here:
                // the tolerance of this solve is lifted above it (bounded by 1e-2) and the search repeated.
                if (bp >= 0) {
                    bool again = false;
#pragma unroll
                    for (int h = 0; h < kHist; ++h) again = again || (bp == hist_bp[h] && fabs(best - hist_best[h]) <= 1e-3 * best);
                    if (again) {
                        double top = best;
#pragma unroll
                        for (int h = 0; h < kHist; ++h) if (hist_bp[h] >= 0 && hist_best[h] > top && hist_best[h] < 1e-2) top = hist_best[h];
                        if (2.0 * top < 1e-2) {
                            tol_floor = 2.0 * top;
#pragma unroll
                            for (int h = 0; h < kHist; ++h) hist_bp[h] = -1;
                            bp = find_violation(L, c, tol_floor, best);
                        }
                    }
                }
                if (bp >= 0) {
#pragma unroll
                    for (int h = kHist - 1; h > 0; --h) { hist_bp[h] = hist_bp[h - 1]; hist_best[h] = hist_best[h - 1]; }
                    hist_bp[0] = bp; hist_best[0] = best;
                }
            }
            PTOC(L, 4);
            if (bp < 0) break;
            if (++st.iters > max_iter) { st.status = 2; break; }
            q.kq = bp >> 5; q.qcode = bp & 31;
            q.is_bound = q.qcode >= 16;
            q.tq = q.is_bound ? 0 : q.qcode;
            q.gq = q.is_bound ? (q.qcode - 16) : ((q.kq == N) ? G_NONE : group_of(q.qcode));
            have_q = true; lam_q = 0.0;
            incoming_row(L, c, q);
        }
        if (++st.events > (kBaseline ? 10 : 40) * max_iter) { st.status = 2; break; }
        const int kq = q.kq;
        const double viol = row_value(q, kq, N, M.av, M.shv, M.vhv, q.d);
        // u = He c_q and its trajectories
        double cj = mb_reduce(L, c, normal_at(L, kq, q.al, q.be, q.ga, q.de, tauv[kq]));
        if (lane < NS) M.yv[lane] = cj;
        WSYNC();
        double u = mb_expand(L, c, he_apply<NS>(Hs, M.yv, N, lane));
        double su, vu;
        hom_traj(L, u, su, vu);
        if (lane < N) M.ub[lane] = u;
        if (lane <= N) { M.sub[lane] = su; M.vub[lane] = vu; }
        WSYNC();
        const double cu = row_value(q, kq, N, M.ub, M.sub, M.vub, 0.0);
        double sr = 0.0;
        if (m > 0) sr = step_rates(M, m, N, lane);
        const double zz = cu - sr;
        double t2 = (zz > 1e-8 * cu) ? viol / zz : kInf;
        if (viol <= 0.0) t2 = 0.0;
        // blocking events, evaluated per (lane, type); multipliers and their rates are read from the
        // working-set list in this lane's order
        double t1 = kInf; int ev = EvCode::kNoEvent;
        {
            // candidate step lengths num / den (den > 0) are compared cross-multiplied against the lane's best so far
            // (t1n / t1d): one division per lane at the end instead of one per candidate
            double t1n = kInf, t1d = 1.0;
#define EEPACC_CAND(NUM, DEN, EVCODE) do { const double _n = (NUM), _d = (DEN); \
                if (_n * t1d < t1n * _d) { t1n = _n; t1d = _d; ev = (EVCODE); } } while (0)
            double sumLF = 0, sumLS = 0, sumLV = 0, sumRF = 0, sumRS = 0, sumRV = 0;
            int pos = L.base;
#pragma unroll
            for (int t = 0; t < kNumRowTypes; ++t) {
                if (!row_live(t)) continue;
                int cd = code_of(L, t);
                if (cd != 1) continue;
                int g2 = lane_group(L, t);
                const double l = M.lam[pos], r = M.rv[pos];
                ++pos;
                const bool blocks = !(pf && l < 0.0);      // primal first: a negative multiplier cannot block the step
                if (g2 == G_H) {
                    // rigid row of the quadratic slack: 0 <= lambda <= w
                    if (r > 0.0) { if (blocks) EEPACC_CAND(fmax(l, 0.0), r, EvCode::pack(EV_DROP, lane, t)); }
                    else if (r < 0.0) EEPACC_CAND(fmax(c.wH - l, 0.0), -r, EvCode::pack(EV_COMPL, lane, t));
                } else {
                    if (r > 0.0 && blocks) EEPACC_CAND(fmax(l, 0.0), r, EvCode::pack(EV_DROP, lane, t));
                    if (g2 == G_F) { sumLF += l; sumRF += r; } else if (g2 == G_S) { sumLS += l; sumRS += r; } else if (g2 == G_V) { sumLV += l; sumRV += r; }
                }
            }
            if (lane < N) {
#pragma unroll
                for (int g2 = G_F; g2 <= G_V; ++g2) {
                    double sl = g2 == G_F ? sumLF : (g2 == G_S ? sumLS : sumLV);
                    double srr = g2 == G_F ? sumRF : (g2 == G_S ? sumRS : sumRV);
                    double rate = -srr, margin = group_w(c, g2) - sl;
                    if (lane == kq && q.gq == g2) { rate += 1.0; margin -= lam_q; }
                    if (rate > 0.0) EEPACC_CAND(fmax(margin, 0.0), rate, EvCode::pack(EV_CAP, lane, g2));
                }
            }
            if (lane == kq && !q.is_bound && q.gq == G_H) EEPACC_CAND(fmax(c.wH - lam_q, 0.0), 1.0, EvCode::pack(EV_CAPIN, lane, 0));
            if (lane == kq && q.is_bound && q.gq == G_H) {
                // incoming slack bound of a penalised row: the row's own multiplier
                // w + q*xi - mu must stay >= 0 while xi rises with the step
                const double xi_now = L.lbH - viol, den = 1.0 - c.qH * zz;
                if (den > 0.0) EEPACC_CAND(fmax(c.wH + c.qH * xi_now - lam_q, 0.0), den, EvCode::pack(EV_DROPH, lane, R_HWP));
            }
#undef EEPACC_CAND
            t1 = (ev == EvCode::kNoEvent) ? kInf : t1n / t1d;
            wave_argmin(t1, ev);
        }
        const double tstep = fmin(t1, t2);
#ifdef EEPACC_BL_TRACE
        if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("it %d ev %d m %d q(k %d code %d b %d) best %.3e viol %.6e zz %.3e cu %.3e lam_q %.6e t1 %.6e t2 %.6e ev(%d,%d,%d) fast %d\n",
                              st.iters, st.events, m, kq, q.qcode, (int)q.is_bound, best, viol, zz, cu, lam_q, t1, t2, ev >> 16, (ev >> 5) & 63, ev & 31, F.fast);
#endif
        if (!(tstep < 1e299) && pf) { have_q = false; lam_q = 0.0; pf = false; pf_left = 0; continue; }      // back to the repair
        if (!(tstep < 1e299)) {
            // the incoming normal lies in the span of the working set and nothing can be dropped.
            // With a real violation the QP is infeasible; with a rounding-level one the row is a
            // duplicate of active rows (e.g. a_k pinned by an acceleration AND a jerk limit): mark it
            // as ignored for this solve.
            if (best < 1e-7) { if (lane == kq) L.ign |= (1u << q.qcode); have_q = false; lam_q = 0.0; WHY(5); continue; }
            st.status = 1; break;
        }
        lam_q += tstep;
        bool finished = false;
        if (t2 <= t1) {
            // full step: the incoming constraint becomes active
            if (!q.is_bound && m > 0) { F.fast = 1; F.kq = kq; F.tq = q.tq; F.zz = zz; }
            WHY(q.is_bound ? 4 : 8);
            if (lane == kq) {
                if (!q.is_bound) set_code(L, q.tq, 1);
                else if (q.gq == G_H) set_code(L, R_HWP, 1);      // penalised row turns rigid
                else { int p = pivot_of(L, q.gq); set_code(L, p, 1); }
            }
            finished = true;
        } else {
            const int ek = EvCode::kind(ev), el = EvCode::lane(ev), et = EvCode::type(ev);
            if (ek == EV_DROP) {
                const int pl = rows_below(L, et);
                F.drop_pos = __builtin_amdgcn_readlane(L.base + pl, __builtin_amdgcn_readfirstlane(el));
                F.fast = 2;
                if (lane == el) set_code(L, et, 0);
            }
            else if (ek == EV_COMPL) { if (lane == el) set_code(L, et, 3); WHY(3); }
            else if (ek == EV_DROPH) {
                if (lane == el) set_code(L, et, 0);
                finished = true; WHY(3);
                // a penalised row whose slack already lies below its bound (a warm state that belongs to another problem:
                // w + q xi < 0, the step length above is clipped to zero) leaves He at once and the slack jumps back onto its
                // bound: discontinuous like EV_CAPIN below, so the multipliers of the working set are re-validated as well
                // (also taken when w + q xi - lam_q is exactly 0 at a right state: harmless, one repair pass)
                if (!(tstep > 0.0)) { warm = true; pass = 0; }
            }
            else if (ek == EV_CAPIN) {
                // the slack jumps off its bound by the remaining violation: the one discontinuous event of the method.
                // The multipliers of the working set are re-validated (repair passes) before the next constraint is
                // looked for; without this a row could be left in the working set with a negative multiplier
                if (lane == el) set_code(L, R_HWP, 3);
                finished = true; warm = true; pass = 0; WHY(3);
            }
            else if (ek == EV_CAP) {
                WHY(2);
                int fin = 0;
                if (lane == el) {
                    const int g2 = et;
                    // members (code 1) of the group with their multipliers after the step
                    int bestm = -1; double bl = -1e300;
                    int pos = L.base;
#pragma unroll
                    for (int t = 0; t < kNumRowTypes; ++t) {
                        if (!row_live(t)) continue;
                        if (code_of(L, t) != 1) continue;
                        const double l = M.lam[pos] - tstep * M.rv[pos];
                        ++pos;
                        if (t >= R_AMAX && t <= R_VINC && group_of(t) == g2 && l > bl) { bl = l; bestm = t; }
                    }
                    const int p = pivot_of(L, g2);
                    const bool q_row_here = (kq == el) && !q.is_bound && q.gq == g2;
                    const bool q_bound_here = (kq == el) && q.is_bound && q.gq == g2;
                    if (p < 0) {                       // Z -> P
                        if (bestm < 0) { set_code(L, q.tq, 2); fin = 1; }
                        else set_code(L, bestm, 2);
                    } else {                           // pivot multiplier reached zero
                        set_code(L, p, 0);
                        if (bestm >= 0) set_code(L, bestm, 2);
                        else if (q_row_here) { set_code(L, q.tq, 2); fin = 1; }
                        else if (q_bound_here) { fin = 1; }
                    }
                }
                if (__any(fin)) finished = true;
            }
        }
        if (F.fast != 0 && carry_ok) {
            // plain row in (F.fast == 1) or out (== 2): group states, penalties and the objective part are unchanged, so
            // the point moves along  z = He (c_q - C' r)  and the multipliers along -r; the list positions follow the
            // lane-major order the next rebuild will produce
            const double y = mb_reduce(L, c, direction_side(L, M, m, kq, q.al, q.be, q.ga, q.de));
            if (lane < NS) M.yv[lane] = y;
            WSYNC();
            const double z = mb_expand(L, c, he_apply<NS>(Hs, M.yv, N, lane));
            double sz, vz;
            hom_traj(L, z, sz, vz);
            L.a = fma(-tstep, z, L.a); L.sh = fma(-tstep, sz, L.sh); L.vh = fma(-tstep, vz, L.vh);
            L.am1 = lane_prev(L.a);
            if (lane < N) M.av[lane] = L.a;
            if (lane <= N) { M.shv[lane] = L.sh; M.vhv[lane] = L.vh; }
            const double lv = (lane < m) ? fma(-tstep, M.rv[lane], M.lam[lane]) : 0.0;
            WSYNC();
            if (F.fast == 1) {
                const int pl = rows_below(L, q.tq);
                const int p = __builtin_amdgcn_readlane(L.base + pl, __builtin_amdgcn_readfirstlane(kq));
                if (lane < m && lane + 1 < MMAX) M.lam[lane < p ? lane : lane + 1] = lv;
                if (lane == 0 && p < MMAX) M.lam[p] = lam_q;
            } else {
                const int dp = F.drop_pos;
                if (lane < m && lane != dp) M.lam[lane < dp ? lane : lane - 1] = lv;
            }
            WSYNC();
            inc_next = true;
        }
        if (finished) { have_q = false; lam_q = 0.0; pf = false; q.al = q.be = q.ga = q.de = q.d = 0.0; }
        PTOC(L, 5);
    }
    if (st.status == 0 && m > 0) refine_primal(L, c, M, Hs, m, 0.0, 0, 0.0, 0.0, 0.0, 0.0, grad_total, 4, 1e-14);
    st.m = m;
    return st;
}

// ----------------------------------------------------------------------------------------------
// per-step set-up: estimator, bounds, right-hand sides (A2, A3, A4 of SURVEY.md section 8a)

struct StepIn { double s, v, a_prev, t0, s_tv, v_tv, a_tv_prev; };

// est: what the caller supplies of the horizon guesses of this lane's stage, in place of the estimators' (ego: s_est and
// v_est, lead: stv_est).  An argument of ab_step in that variant alone.
struct EstIn { bool ego, lead; double s_est, v_est, stv_est; };

// ABO/RunOpt_ABMPC.m:287-324
__device__ void force_allocation(const DevCfg& C, double s_meas, double v_meas, double a_qp,
                                 double& Fm, double& Fb, double& a_real) {
    double sn, cs;
    slope_trig(C, s_meas, sn, cs);
    double F_r = -C.zeta_a * v_meas * v_meas - C.c_r * C.m * C.g * cs - C.m * C.g * sn;
    double F_t_req = C.m * C.lambda * a_qp - F_r;
    double F_f_r_max = C.mu / C.L * (C.m * C.g * (C.L_f * cs + C.h_g * sn) +
                                     C.h_g * (C.zeta_a * v_meas * v_meas + C.lambda * C.m * a_qp));
    double F_f_tot_max = C.mu * C.m * C.g * cs;
    if (F_t_req < 0.0) {
        double F_m_min = (v_meas < C.omega_m_r / C.phi) ? -C.phi * C.T_m_max / C.eta_TF : -C.P_m_max / C.eta_TF / v_meas;
        double fm = fmax(fmax(F_t_req, F_m_min), -F_f_r_max);
        Fm = fm;
        Fb = fmax(F_t_req, -F_f_tot_max) - fm;
    } else {
        double F_m_max = (v_meas < C.omega_m_r / C.phi) ? C.phi * C.T_m_max * C.eta_TF : C.P_m_max * C.eta_TF / v_meas;
        Fm = fmin(fmin(F_t_req, F_m_max), F_f_r_max);
        Fb = 0.0;
    }
    a_real = (Fm + Fb + F_r) / C.m / C.lambda;
}

// ICE-map variant with move blocking: Hbar = E'HE in the leader-indexed layout the host builds for the withmb kernels
// (eepacc_capi.cpp): on each leader row / column H summed over the block, identity on the non-leader rows.  Lane b, the
// leader of a block, forms the entries (a, b) of every leader a (a >= b when packed) from the block pair and then writes
// unit / zero on the pair's non-leader rows and columns; the block pairs partition the matrix, so the lanes work in place.
template <int NS>
__device__ __forceinline__ void he_mb_fold(double* He, const Cfg& c, int N, int lane) {
    auto at = [](int i, int j) { return kPackedHe<NS> ? (i >= j ? he_tri(i) + j : he_tri(j) + i) : i * NS + j; };
    if (lane < N && c.mb_lead[lane] == lane) {
        const int b = lane, be = c.mb_end[b];
        for (int a = kPackedHe<NS> ? b : 0; a < N; a = c.mb_end[a] + 1) {
            const int ae = c.mb_end[a];
            double s = 0.0;
            for (int i = a; i <= ae; ++i)
                for (int j = b; j <= be; ++j) s += He[at(i, j)];
            for (int i = a; i <= ae; ++i)
                for (int j = b; j <= be; ++j)
                    if (!kPackedHe<NS> || i >= j) He[at(i, j)] = (i == a && j == b) ? s : (i == j ? 1.0 : 0.0);
        }
    }
    WSYNC();
}

// Packed lower triangle of NS = 64 spread evenly over the lanes: column p = lane % 32 (64 - p entries) is paired with
// column 63 - p (p + 1 entries); of the pair's 65 entries, lanes 0-31 take the first 33 and lanes 32-63 the other 32.
// Entry u of this lane is (i, j); false where the lane has no entry u.
__device__ __forceinline__ bool he_pair_entry(int lane, int u, int& i, int& j) {
    const int p = lane & 31, t = (lane >> 5) * 33 + u;
    if (t < 64 - p) { i = p + t; j = p; } else { i = t - 1; j = 63 - p; }
    return t <= 64;
}
constexpr int kPairEntries = 33;

// ICE-map Hessian at NS = 64 (the small path in ab_step, on the packed triangle): build H from the closed forms into He
// (M.ws = Rsuf, the suffix sums of cq_k), fold it for move blocking, invert it in place by symmetric sweeps (the pivot row
// staged in M.wa) and write the negated result, the step's base inverse, to the wave's scratch Hb (full N x N).
// Returns 1 when a pivot is not positive (status 2).
template <int MMAX, int NS>
__device__ __forceinline__ int ice_build_invert_packed(const DevCfg& C, const Cfg& c, WaveMem<MMAX, NS>& M, double* He,
                                                       double* __restrict__ Hb, int N, int lane) {
    static_assert(NS == 64, "the lane pairing covers the 64 x 64 triangle");
    if (lane < NS) M.wv[lane] = lane < N ? C.Tvec[lane] : 0.0;
    WSYNC();
    // jerk weights q_k = 2 w_j / T_k^2 of the two columns this lane's entries lie in (and of the stage after each)
    const int p = lane & 31;
    auto qj = [&](int k) { return k < N ? 2.0 * C.w_j / (M.wv[k] * M.wv[k]) : 0.0; };
    const double qA0 = qj(p), qA1 = qj(p + 1), qB0 = qj(63 - p), qB1 = qj(64 - p);
#pragma unroll 1
    for (int u = 0; u < kPairEntries; ++u) {
        int i, j;
        if (!he_pair_entry(lane, u, i, j)) continue;
        double hv = 0.0;
        if (i < N) {
            const double q0 = j == p ? qA0 : qB0, q1 = j == p ? qA1 : qB1;
            hv = 2.0 * M.wv[i] * M.wv[j] * M.ws[i];
            if (i == j) hv += 2.0 * C.w_a + q0 + q1;
            else if (i == j + 1) hv -= q1;
        }
        He[he_tri(i) + j] = hv;
    }
    WSYNC();
    if (kMoveBlocking && c.mb_len != 0) he_mb_fold<NS>(He, c, N, lane);
    int bad = 0;
    for (int k = 0; k < N; ++k) {
        const double d = He[he_tri(k) + k];
        if (!(d > 0.0)) { bad = 1; break; }
        const double inv = 1.0 / d;
        if (lane < NS) M.wa[lane] = lane < N ? He[lane >= k ? he_tri(lane) + k : he_tri(k) + lane] : 0.0;
        WSYNC();
        const double fA = M.wa[p] * inv, fB = M.wa[63 - p] * inv;
#pragma unroll 3
        for (int u = 0; u < kPairEntries; ++u) {
            int i, j;
            if (!he_pair_entry(lane, u, i, j) || i >= N) continue;
            const int e = he_tri(i) + j;
            const double f = j == p ? fA : fB, ck = M.wa[i], old = He[e];
            He[e] = (i == k) ? (j == k ? -inv : f) : (j == k ? ck * inv : fma(-ck, f, old));
        }
        WSYNC();
    }
#pragma unroll 1
    for (int u = 0; u < kPairEntries; ++u) {
        int i, j;
        if (!he_pair_entry(lane, u, i, j) || i >= N) continue;
        const int e = he_tri(i) + j;
        const double x = -He[e];
        He[e] = x;
        Hb[i * N + j] = x;                   // base inverse of this step (cold restarts re-read it)
        Hb[j * N + i] = x;
    }
    return bad;
}

// One ABMPC step for the wave's instance (ABO/RunOpt_ABMPC.m:193-329).  `code` carries the
// working set between steps (already shifted by the caller).
template <int MMAX, int NS, class... Est>
__device__ __forceinline__ void ab_step(const DevCfg& C, WaveMem<MMAX, NS>& M, double* Hs, const StepIn& in,
                        unsigned long long& code, StepOut& so, double& s_pred, double& v_pred,
                        const double* predp, bool pred_in_lds, double* Hb, Est... est) {
    static_assert(sizeof...(Est) == (kEst ? 1 : 0), "supplied guesses are an argument of the est kernels, and of them alone");
    Lane L;
#ifdef EEPACC_AB_TIMING
    for (int i = 0; i < 24; ++i) L.prof[i] = 0;
    long long _t0 = wall_clock64();
#endif
    L.lane = lane_id(); L.N = C.N;
    const int lane = L.lane, N = C.N;
    const int kk = lane <= N ? lane : N;
#ifdef EEPACC_BL_TRACE
    if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("--- step t0 %.2f s %.4f v %.5f s_tv %.4f v_tv %.4f warm rows %d\n", in.t0, in.s, in.v, in.s_tv, in.v_tv, (int)__popcll(codes_eq1(code)));
#endif
    L.T = lane < N ? C.Tvec[lane] : 0.0;
    L.tau = C.tau[kk];
    L.tau1 = C.tau[kk + (lane < N ? 1 : 0)];
    L.tau_rev = C.tau[lane <= N ? N - lane : 0];
    Cfg c;
    c.N = N; c.tau_min = C.tau_min; c.wF = C.w_f; c.wS = C.w_s; c.wV = C.w_v; c.wH = 100.0 * C.w_h; c.qH = 2.0 * C.w_h;
    c.mb_len = C.mb_any ? C.mb_maxlen : 0; c.mb_lead = C.mb_lead; c.mb_end = C.mb_end;
    // estimators (A2)
    double s_est, v_est, stv_est, vtv_est;
    if (C.paramEstSetting == 2) {
        // EstimateVehicleTrajectory.m:81-88: shifted previous solution, [x_curr; prev(3:end); prev(end) + Ts v_prev(end)]
        // (previous z(1:7:end), z(2:7:end) kept in LDS between the steps of a launch, in C.pred across launches)
        const int idx = lane < N ? lane + 1 : N;
        const double ps = pred_in_lds ? M.ws[idx] : predp[idx], pv = pred_in_lds ? M.wv[idx] : predp[64 + idx];
        s_est = lane == 0 ? in.s : (lane < N ? ps : ps + C.Tvec[N - 1] * pv);
        v_est = lane == 0 ? in.v : pv;
        WSYNC();
    } else {
        estimate_traj(C, C.paramEstSetting, C.tConstACC_ego, in.s, in.v, in.a_prev, lane, s_est, v_est);
    }
    // (target-vehicle MPC: no lead vehicle, RunOpt_TVMPC.m:157 estimates its own trajectory only)
    if constexpr (kTargetVeh) { stv_est = 0.0; vtv_est = 0.0; }
    else estimate_traj(C, C.TVestSetting, C.tConstACC_tar, in.s_tv, in.v_tv, in.a_tv_prev, lane, stv_est, vtv_est);
    if constexpr (kEst) {
        // CreateQP_AB takes s_est, v_est and s_tv_est as inputs: what the caller supplied stands in place of the estimate
        const EstIn e[] = {est...};
        if (e[0].ego) { s_est = e[0].s_est; v_est = e[0].v_est; }
        if (e[0].lead) stv_est = e[0].stv_est;
    }
    const double dist_hor = bcast(s_est, N) - in.s;                          // :200
    const double stv_Nm1 = kTargetVeh ? 0.0 : bcast(stv_est, N - 1);
    // bounds (A3)
    double v_lim, v_curv, v_stop, v_TL, a_min, a_max, j_min, j_max;
    // CreateQP_TV.m:44-45 hands EstimateRouteAndComfortBounds v_est = zeros: of :63-208 only the gear estimate (unused by
    // CreateQP_TV) and the comfort limits read v_est, and at 0 < 5 m/s those are the low-speed limits at every stage
    route_bounds(C, s_est, kTargetVeh ? 0.0 : v_est, in.t0, lane < N ? lane : N - 1, v_lim, v_curv, v_stop, v_TL, a_min, a_max, j_min, j_max);
    if constexpr (kTargetVeh) { v_lim *= 0.8; v_curv *= 0.8; }              // CreateQP_TV.m:265,271 (stop and traffic-light caps unscaled)
    const double T_hwp = 2.0, A_hwp = 2.0, G_hwp = -0.0246 * T_hwp + 0.010819;
    L.chw = T_hwp + G_hwp * v_est;
    // free response of the double integrator and a-space right-hand sides (A4 + A5)
    const double sf = in.s + L.tau * in.v, vf = in.v;
    double b[kNumRowTypes];
    b[R_SLO] = -0.0; b[R_SHI] = C.s_goal; b[R_VLO] = -0.0; b[R_VHI] = C.v_max;
    b[R_AMAX] = a_max; b[R_AMIN] = -a_min;
    b[R_JMAX] = L.T * j_max + (lane == 0 ? in.a_prev : 0.0);
    b[R_JMIN] = -(L.T * j_min + (lane == 0 ? in.a_prev : 0.0));
    b[R_VLIM] = v_lim; b[R_VCURV] = v_curv; b[R_VSTOP] = v_stop; b[R_VTL] = v_TL;
    if constexpr (!kTargetVeh) {
        b[R_VINC] = -fmin(v_lim, v_curv);
        b[R_SAFE1] = stv_est - C.h_min; b[R_SAFE2] = stv_est; b[R_HWP] = stv_est - A_hwp;
        if (lane == N) { b[R_SAFE1] = stv_Nm1 - C.h_min; b[R_SAFE2] = stv_Nm1; }
    }
    unsigned valid = 0u;
    L.lbF = L.lbS = L.lbV = L.lbH = 0.0;
    int infeasible_const = 0;
#pragma unroll
    for (int t = 0; t < kNumRowTypes; ++t) {
        if (!row_live(t)) continue;
        double al = row_al(t), be = row_be(t, c.tau_min, L.chw);
        L.ba[t] = b[t] - al * sf - be * vf;
        bool exists;
        if (lane < N) {
            exists = true;
            if (t == R_SHI && !(C.s_goal < 1e300)) exists = false;
            if ((t == R_VLIM || t == R_VCURV || t == R_VSTOP || t == R_VTL) && !C.ab_route_rows) exists = false;
            if (kBaseline && (t == R_VINC || t == R_HWP)) exists = false;
        } else exists = (lane == N) && (t == R_SAFE1 || t == R_SAFE2);      // (CreateQP_TV.m:288-292: no terminal rows; skipped above)
        // a supplied guess may say "no lead" (+inf) at a stage where the carried working set, made on another guess, holds a
        // lead row: such a row does not exist, so that its code is dropped below instead of entering the solve with an infinite bound
        // (blest: SAFE1 and SAFE2 belong to the one slack group; a group whose pivot is dropped here is back at its bound, the
        // state every shifted code of lane 0 is left in already, and the violation search, slide_limit and the LP's proximal
        // re-solves read L.valid, so none of them sees the row)
        if constexpr (kEst) { if ((t == R_SAFE1 || t == R_SAFE2 || t == R_HWP) && !(b[t] < kInf)) exists = false; }
        if (exists && lane == 0 && row_ga(t) == 0.0) {
            // stage-0 rows without an a-component are constants: fold into slack bounds
            exists = false;
            int g2 = group_of(t);
            double need = -L.ba[t];
            // hard constant row (bounds on the measured s_0, v_0): infeasible beyond state_bound_tol (default 1e-9: the
            // plant's rounding noise at standstill, |v| ~ 1e-10, is let through -- every saved ABMPC solution has
            // exitMessage = 0 there; the reference's LP solve of the baseline controller gave up on v_0 = -3e-10, which
            // state_bound_tol = 1e-11 reproduces)
            if (g2 == G_NONE) { if (need > C.state_tol) infeasible_const = 1; }
            else if (g2 == G_F) L.lbF = fmax(L.lbF, need);
            else if (g2 == G_S) L.lbS = fmax(L.lbS, need);
            else if (g2 == G_V) L.lbV = fmax(L.lbV, need);
            else L.lbH = fmax(L.lbH, need);
        }
        if (exists) valid |= (1u << t);
    }
    L.valid = valid;
    L.ign = 0u;
    // drop warm-start codes of rows that do not exist at this lane
    L.code = code;
#pragma unroll
    for (int t = 0; t < kNumRowTypes; ++t)
        if (!((valid >> t) & 1u)) set_code(L, t, 0);
    // base gradient (condensed objective, CreateQP_AB.m:162-180 through Psi'):
    //   g_j = T_j * (N-1-j) * (2 cq v0 + w_FC p10) + w_FC p01 lambda m ; g_0 -= 2 w_j/T_0 a_{-1}
    L.g0 = 0.0;
    if (lane < N) {
        // (baseline: -w_v on v_k for k = 0..N, CreateQP_BL.m:139,318: the terminal stage counts too)
        L.g0 = L.T * (double)(N - (kBaseline ? 0 : 1) - lane) * (2.0 * C.cq * in.v + C.glin_v) + C.glin_a;
        if (lane == 0) L.g0 -= 2.0 * C.w_j / L.T * in.a_prev;
    }
    L.a = L.sh = L.vh = L.am1 = 0.0;
    double grad_total = 0.0;
    const double* Hbase = C.Hinv;
    int h_bad = 0;
    if constexpr (kIce) {
        // ICE-map fuel term (CreateQP_AB.m:154-159): stage k carries the curvature 2 cq_k on v_k and the linear terms
        // lv_k v_k + la_k a_k with the gear ratio tau_est(k) = LUTgearshift(v_est(k)) (LUTgearshift.m:17-41,
        // EstimateRouteAndComfortBounds.m:63-66).  v_k = v_0 + sum_{i<k} T_i a_i, so
        //   g_j = T_j sum_{k>j} (2 cq_k v_0 + lv_k) + la_j,   H_ij = 2 T_i T_j sum_{k>max(i,j)} cq_k + (acceleration, jerk)
        // change every step: closed forms from two suffix sums, inverse in LDS by symmetric sweeps
        double tg = C.ice_gb[7];
#pragma unroll
        for (int g2 = 6; g2 >= 0; --g2) if (v_est < C.ice_up[g2]) tg = C.ice_gb[g2];
        const bool stg = lane < N;
        const double cqk = stg ? C.ice_cq / tg : 0.0, lvk = stg ? C.ice_lv * tg : 0.0, lak = stg ? C.ice_la / tg : 0.0;
        const bool dep = stg && lane > 0;                                   // v_0 is the measured state
        const double wi = scan_incl(dep ? 2.0 * cqk * in.v + lvk : 0.0), ci = scan_incl(dep ? cqk : 0.0);
        const double Wsuf = read_lane63(wi) - wi, Rsuf = read_lane63(ci) - ci;      // sums over the stages > lane
        if (stg) { L.g0 = L.T * Wsuf + lak; if (lane == 0) L.g0 -= 2.0 * C.w_j / L.T * in.a_prev; }
        if (lane <= N) M.ws[lane] = Rsuf;
        WSYNC();
        if constexpr (kPackedHe<NS>) {
            h_bad = ice_build_invert_packed<MMAX, NS>(C, c, M, Hs, Hb, N, lane);
        } else {
            if (lane < NS) {
                const int j = lane;
                const double Tj = j < N ? C.Tvec[j] : 0.0;
                const double qjj = j < N ? 2.0 * C.w_j / (Tj * Tj) : 0.0;
                const double qjn = (j + 1 < N) ? 2.0 * C.w_j / (C.Tvec[j + 1] * C.Tvec[j + 1]) : 0.0;
                for (int i = 0; i < NS; ++i) {
                    double hv = 0.0;
                    if (i < N && j < N) {
                        hv = 2.0 * C.Tvec[i] * Tj * (i > j ? M.ws[i] : Rsuf);
                        if (i == j) hv += 2.0 * C.w_a + qjj + qjn;
                        else if (i == j - 1) hv -= qjj;
                        else if (i == j + 1) hv -= qjn;
                    }
                    Hs[i * NS + j] = hv;
                }
            }
            WSYNC();
            if (kMoveBlocking && c.mb_len != 0) he_mb_fold<NS>(Hs, c, N, lane);
            h_bad = he_invert_full<NS>(Hs, M.wa, N, lane);
            for (int e = lane; e < NS * NS; e += 64) {
                const double x = -Hs[e];
                Hs[e] = x;
                const int i = e / NS, j = e % NS;
                if (i < N && j < N) Hb[i * N + j] = x;           // base inverse of this step (cold restarts re-read it)
            }
        }
        Hbase = Hb;
    } else {
        // per-wave inverse of the effective Hessian: start from the step-invariant H^-1
        he_load_base<NS>(Hs, C.Hinv, N, lane);
    }
    L.kmask = 0ull;
    WSYNC();
#ifdef EEPACC_AB_TIMING
    L.prof[6] += wall_clock64() - _t0;
    _t0 = wall_clock64();
#endif
    // Crash start of an empty working set: the travel-incentive slack (one row per stage, its own group) of every stage that
    // is slower than the incentive speed at the zero-acceleration trajectory starts off its bound.  The dual iteration would
    // reach that state one stage per iteration (measured: 29 of the 51 working-set changes of a first step); a stage where
    // it is wrong shows up as a violated slack bound, like any other wrong state.
    if constexpr (!kBaseline) {
        if (!__any(L.code != 0ull)) {
            if (lane < N && ((L.valid >> R_VINC) & 1u) && row_val(L, c, R_VINC, L.ba[R_VINC]) > L.lbV) set_code(L, R_VINC, 2);
        }
    }
    // baseline controller: a solve that fails from a warm working set (a degenerate vertex of the LP can leave the
    // shifted set numerically dependent) is repeated once from the empty one before the step is reported as failed
    // (compiled into that variant only: the loop costs the ABMPC kernels registers, and their tests never need it)
#ifdef EEPACC_BL_TRACE
    if ((gridDim.x == 1 || g_trace_on) && lane <= N) printf("   start code[%2d] %016llx\n", lane, L.code);
#endif
    const bool had_warm = kBaseline && __any(L.code != 0ull) != 0;
    SolveStats st{0, 0, 0, 0};
    for (int attempt = 0; attempt < (kBaseline ? 2 : 1); ++attempt) {
        if (kIce && h_bad) { st.status = 2; break; }
        st = solve_qp<MMAX, NS>(L, c, M, Hs, Hbase, C.tau, C.max_iter, grad_total);
        if (st.status == 0 || !had_warm || attempt == 1 || st.iters > C.max_iter / 2) break;      // (a cycling solve is not repeated)
        L.code = 0ull; L.ign = 0u;
        L.a = L.sh = L.vh = L.am1 = 0.0;
        he_load_base<NS>(Hs, Hbase, N, lane);
        L.kmask = 0ull;
        WSYNC();
    }
    // Baseline controller, linear program: the curvature bl_eps that the dual active set needs is applied as a PROXIMAL term
    // bl_eps/2 |a - a_j|^2 around the previous solution (a_0 = 0) and the solve repeated from its own working set until the
    // point stays: for a linear program the proximal-point iteration ends after finitely many steps at an optimum of the
    // LP itself, for any bl_eps.  That is what allows bl_eps = 1e-2 instead of 1e-4: with multipliers of w_f = 1e7 the row
    // values carry a rounding noise of about 1e-13 * w_f / bl_eps, which at 1e-4 (1e-3 m) made degenerate standstill
    // vertices cycle; most steps need the one confirming solve only (no working-set change).
    double centre = 0.0;
    [[maybe_unused]] int prox_used = 0;
    if constexpr (kBaseline) {
        if (C.bl_eps > 0.0 && C.bl_prox_max > 0 && st.status == 0) {
            const double g0_lp = L.g0;
            double next_centre = (lane < N) ? L.a : 0.0;
            for (int pit = 0; pit < C.bl_prox_max; ++pit) {
                centre = next_centre;
                L.g0 = g0_lp - C.bl_eps * centre;
                const SolveStats s2 = solve_qp<MMAX, NS>(L, c, M, Hs, Hbase, C.tau, C.max_iter, grad_total);
                st.iters += s2.iters; st.events += s2.events; st.m = s2.m;
                prox_used = pit + 1;
                if (s2.status != 0) { st.status = s2.status; break; }
                const double delta = (lane < N) ? L.a - centre : 0.0;
                double d = fabs(delta), amax = (lane < N) ? fabs(L.a) : 0.0;
                int dummy = lane;
                wave_argmax(d, dummy);
                wave_argmax(amax, dummy);
                if (d <= 1e-7 * (1.0 + amax)) break;          // the point stays where its centre is: an optimum of the LP
                next_centre = (lane < N) ? L.a : 0.0;
                double tlim = 0.0;
                if (s2.iters == 0 && s2.events == 0) {
                    // No working-set state changed: the iteration slid along an edge of the LP by delta = -(reduced cost) / bl_eps,
                    // and every further re-centring would add the same delta (same multipliers) until a row outside the
                    // working set comes up.  Those iterations are taken at once: the next centre is the last one before that row.
                    Lane L0 = L;
                    L0.a = centre;
                    hom_traj(L0, centre, L0.sh, L0.vh);
                    L0.am1 = dpp_zero<0x138, 0xf>(L0.a);
                    tlim = slide_limit(L, L0, c);
                    if (tlim > 1.0) next_centre = (lane < N) ? fma(fmin(tlim, 1e9) - 1.0, delta, L.a) : 0.0;
                }
#ifdef EEPACC_BL_TRACE
                if (lane == 0 && (gridDim.x == 1 || g_trace_on)) printf("prox %d: |da| %.3e iters %d events %d slide %.3e\n", pit, d, s2.iters, s2.events, tlim);
#endif
            }
        }
    }
#ifdef EEPACC_AB_TIMING
    L.prof[8] += wall_clock64() - _t0;
    _t0 = wall_clock64();
#endif
#ifdef EEPACC_BL_TRACE
    if ((gridDim.x == 1 || g_trace_on) && lane <= N) printf("   end code[%2d] %016llx a %.4f\n", lane, L.code, L.a);
#endif
    code = L.code;
    // recover z = Psi x + d (A7): predicted states
    s_pred = sf + L.sh; v_pred = vf + L.vh;
    // stage-0 slacks and the dense-QP objective value
    double xiF = 0, xiS = 0, xiV = 0, xiH = 0;
    if (lane < N) {
        xiF = fmax(group_xi(L, c, G_F), L.lbF);
        xiS = fmax(group_xi(L, c, G_S), L.lbS);
        xiV = fmax(group_xi(L, c, G_V), L.lbV);
        xiH = EEPACC_HWP_ON(L) ? fmax(row_val(L, c, R_HWP, L.ba[R_HWP]), L.lbH) : L.lbH;
    }
    // 1/2 a'Ha + g'a with H a = -(grad_total - g0) - g0 ... : H a = -grad_total  => a'(g0 - grad/2)
    // 1/2 a'Ha = 1/2 a'H_eff a - q/2 sum_K (n_k'a)^2 and H_eff a = -grad_total
    double part = (lane < N) ? L.a * (L.g0 - 0.5 * grad_total) : 0.0;
    if (kBaseline && lane < N) part += C.bl_eps * L.a * (centre - 0.5 * L.a);      // the LP's proximal term is not part of sol.cost
    part += C.w_f * xiF + C.w_s * xiS + C.w_v * xiV + c.wH * xiH + 0.5 * c.qH * xiH * xiH;
    if (lane < N && EEPACC_HWP_ON(L)) {
        const double na = row_val(L, c, R_HWP, L.ba[R_HWP]) + L.ba[R_HWP];      // n_k'a
        part -= 0.5 * c.qH * na * na;
    }
    const double cost = wave_sum(part);
    const double a0 = bcast(L.a, 0);
    double Fm, Fb, a_real;
    force_allocation(C, in.s, in.v, a0, Fm, Fb, a_real);
    so.out[EEPACC_OUT_S] = in.s;
    so.out[EEPACC_OUT_V] = in.v;
    so.out[EEPACC_OUT_FM] = Fm;
    so.out[EEPACC_OUT_FB] = Fb;
    so.out[EEPACC_OUT_A] = a_real;
    so.out[EEPACC_OUT_XI_V] = bcast(xiV, 0);
    so.out[EEPACC_OUT_XI_H] = bcast(xiH, 0);
    so.out[EEPACC_OUT_XI_S] = bcast(xiS, 0);
    so.out[EEPACC_OUT_XI_F] = bcast(xiF, 0);
    so.out[EEPACC_OUT_COST] = cost;
    so.out[EEPACC_OUT_DISTHOR] = dist_hor;
    so.out[EEPACC_OUT_AQP] = a0;
    so.status = (st.status != 0 || __any(infeasible_const)) ? 1 : 0;
#ifdef EEPACC_DEBUG_STATUS
    if (so.status) so.status = st.status * 100000 + (__any(infeasible_const) ? 10000 : 0) + (st.m + 100) + 1000 * 0;
#endif
#ifdef EEPACC_DEBUG_STATUS
    so.iters = st.iters + 100000 * st.status + 1000000 * (__any(infeasible_const) ? 1 : 0) + 10000000 * st.m;
#elif defined(EEPACC_BL_TRACE)
    so.iters = st.iters + 10000 * prox_used;
#else
    so.iters = st.iters;
#endif
#ifdef EEPACC_AB_TIMING
    L.prof[7] += wall_clock64() - _t0;
    if (L.lane == 0)
        for (int i = 0; i < 24; ++i) atomicAdd(&g_ab_prof[i], (unsigned long long)L.prof[i]);
#endif
}

// LDS layout of a block: per wave [WaveMem][He: N x N doubles]
__host__ __device__ inline size_t wave_bytes(size_t wm, int ns) {
    const size_t he = ns > 32 ? (size_t)ns * (ns + 1) / 2 : (size_t)ns * ns;      // kHeDoubles<NS>
    return ((wm + he * sizeof(double)) + 15) & ~(size_t)15;
}

template <int MMAX, int NS>
__device__ WaveMem<MMAX, NS>* wave_mem(unsigned char* smem, int N, double*& He) {
    unsigned char* base = smem + wave_bytes(sizeof(WaveMem<MMAX, NS>), NS) * (threadIdx.x >> 6);
    He = reinterpret_cast<double*>(base + sizeof(WaveMem<MMAX, NS>));
    return reinterpret_cast<WaveMem<MMAX, NS>*>(base);
}

// The settings of instance b.  The kernels of a handle with settings classes take one more argument than the others, the
// class map of the launch (class_of, values checked by eepacc_set_classes), and their Cp is the handle's class array.  One
// wave serves one instance, and the index is made wave-uniform by construction so that every read of the instance's DevCfg
// stays a scalar load.  N, Tvec and with them the LDS layout are the same in every class (eepacc_create_classes): what is
// fixed for the launch comes from C0 = Cp[0], the head of the array.  The other variants have no such argument (the pack is empty) and keep their
// signature: even an argument they never read moves the kernel's hidden arguments and with them its register allocation.
// In the closed loop a wave serves another instance in every work unit, so the class kernels bind C once more inside the
// unit's body.  That line is a macro and empty in the other variants: bound through cfg_of there too, the same machine code
// comes out for k_ab_step but not for k_run_abmpc (the addresses of the DevCfg arrays are then formed in another order,
// which moves the spills of the N <= 32 kernel), and those kernels are to stay what they were.
#undef EEPACC_AB_UNIT_CFG
#ifdef EEPACC_IMPL_CLASS_MAP
#define EEPACC_AB_UNIT_CFG const DevCfg& C = cfg_of(*Cp, b, extra...);
#else
#define EEPACC_AB_UNIT_CFG
#endif
static_assert(kClasses ==
#ifdef EEPACC_IMPL_CLASS_MAP
              true,
#else
              false,
#endif
              "EEPACC_IMPL_CLASS_MAP is defined for the instantiation whose list entry sets EEPACC_IMPL_CLS, and for no other");
// clsest, blclsest: the kernels' pack holds both, the class map first and the est arguments behind it.  cfg_of (and with it
// EEPACC_AB_UNIT_CFG) takes the whole pack and reads its head; est_supplied / est_preview below take the whole pack too and
// read what follows the map.
template <class Head, class... Tail>
__device__ __forceinline__ Head pack_head(Head head, Tail...) { return head; }
template <class... Extra>
__device__ __forceinline__ const DevCfg& cfg_of(const DevCfg& C0, int b, Extra... extra) {
    static_assert(kEst || sizeof...(Extra) == (kClasses ? 1 : 0), "the class map is an argument of the class kernels, and of them alone");
    if constexpr (kClasses) {
        const int32_t* map = pack_head(extra...);
        return (&C0)[__builtin_amdgcn_readfirstlane(map[b])];
    } else return C0;
}

// est: the further arguments of the two kernels, and what this lane's stage gets of them.  Lane k loads stage k of every
// supplied array ([N_hor+1][B]: one load per array per step, B doubles apart between lanes).  Row N_hor of s_tv_est is not
// read: the terminal rows use s_tv_est(N) of the reference, stage N - 1 here (CreateQP_AB.m:376-387).
__device__ __forceinline__ EstIn est_supplied(int lane, int N, int B, int b, const double* __restrict__ s_est,
                                              const double* __restrict__ v_est, const double* __restrict__ s_tv_est) {
    EstIn e{s_est != nullptr, s_tv_est != nullptr, 0.0, 0.0, 0.0};
    const size_t ke = lane <= N ? lane : N, kl = lane < N ? lane : N - 1;
    if (e.ego) { e.s_est = s_est[ke * B + b]; e.v_est = v_est[ke * B + b]; }
    if (e.lead) e.stv_est = s_tv_est[kl * B + b];
    return e;
}
// (clsest, blclsest: the pack's head is the class map, which cfg_of has read)
__device__ __forceinline__ EstIn est_supplied(int lane, int N, int B, int b, const int32_t* /*class_of*/, const double* __restrict__ s_est,
                                              const double* __restrict__ v_est, const double* __restrict__ s_tv_est) {
    return est_supplied(lane, N, B, b, s_est, v_est, s_tv_est);
}
// The lead's guess of the step at row kk of the launch's traces [n_lead][B], read from the traces themselves
// (eepacc_run_abmpc_preview; scenarios.lead_preview is the specification).  Stage k looks tau_k ahead, at row
// kk + idx[k] + frac[k] (tables of the handle, eepacc::preview_tables): the sample itself where frac is 0, else the two
// neighbours interpolated, and past the last row that row carried on at its speed.  Products and sums are rounded one by
// one, as the specification's are.
__device__ __forceinline__ EstIn est_preview(const DevCfg& C, int lane, int B, int b, int kk, const double* __restrict__ s_tv,
                                             const double* __restrict__ v_tv, const int32_t* __restrict__ idx,
                                             const double* __restrict__ frac, int n_lead) {
    EstIn e{false, true, 0.0, 0.0, 0.0};
    const int k = lane < C.N ? lane : C.N - 1, last = n_lead - 1;
    const int i = kk + idx[k];
    const double f = frac[k];
    if (i < last || (i == last && f == 0.0)) {
        const double a = s_tv[(size_t)i * B + b];
        e.stv_est = f == 0.0 ? a : __dadd_rn(__dmul_rn(1.0 - f, a), __dmul_rn(f, s_tv[(size_t)(i + 1) * B + b]));
    } else {
        const double dt = __dsub_rn(C.tau[k], __dmul_rn((double)(last - kk), C.Tvec[0]));
        e.stv_est = __dadd_rn(s_tv[(size_t)last * B + b], __dmul_rn(v_tv[(size_t)last * B + b], dt));
    }
    return e;
}
// (clsest, blclsest: the class map in front.  C is the DevCfg of the unit's instance, EEPACC_AB_UNIT_CFG's binding: N, tau
// and Tvec[0] are read from it, while idx and frac are the handle's tables, made of class 0's Tvec.  The classes of a
// handle share N and Tvec, so the two agree.)
__device__ __forceinline__ EstIn est_preview(const DevCfg& C, int lane, int B, int b, int kk, const double* __restrict__ s_tv,
                                             const double* __restrict__ v_tv, const int32_t* /*class_of*/, const int32_t* __restrict__ idx,
                                             const double* __restrict__ frac, int n_lead) {
    return est_preview(C, lane, B, b, kk, s_tv, v_tv, idx, frac, n_lead);
}

// B2: one step for B instances.  state: per instance 64 x uint64 codes (instance-major).  extra: the class map (cls), the
// three supplied arrays (est), the map and then the arrays (clsest), nothing elsewhere.
template <int MMAX, int NS, int WPB, class... Extra>
__global__ void __launch_bounds__(64 * WPB, ((NS <= 32 && WPB >= 4) ? 2 : 1))
k_ab_step(const DevCfg* __restrict__ Cp, int B,
          const double* __restrict__ s, const double* __restrict__ v, const double* __restrict__ a_prev,
          const double* __restrict__ t0, const double* __restrict__ s_tv, const double* __restrict__ v_tv,
          const double* __restrict__ a_tv_prev, unsigned long long* __restrict__ codes,
          double* __restrict__ out, double* __restrict__ s_pred, double* __restrict__ v_pred,
          int32_t* __restrict__ status, int32_t* __restrict__ iters, Extra... extra) {
    extern __shared__ __align__(16) unsigned char smem[];
    rc_table_init<MMAX>();
    const int b = blockIdx.x * WPB + (threadIdx.x >> 6);
    if (b >= B) return;
    const DevCfg& C = cfg_of(*Cp, b, extra...);
    double* Hs;
    WaveMem<MMAX, NS>& M = *wave_mem<MMAX, NS>(smem, C.N, Hs);
    const int lane = lane_id();
    StepIn in{s[b], v[b], a_prev[b], t0[b], 0.0, 0.0, 0.0};
    if constexpr (!kTargetVeh) { in.s_tv = s_tv[b]; in.v_tv = v_tv[b]; in.a_tv_prev = a_tv_prev[b]; }       // (no lead inputs: the launcher passes none)
    unsigned long long code = codes[(size_t)b * 64 + lane];
    StepOut so;
    double sp, vp;
    double* predp = C.pred + (size_t)b * 128;
    if constexpr (kEst)
        ab_step<MMAX, NS>(C, M, Hs, in, code, so, sp, vp, predp, false, nullptr, est_supplied(lane, C.N, B, b, extra...));
    else
    ab_step<MMAX, NS>(C, M, Hs, in, code, so, sp, vp, predp, false,
                      kIce ? C.hb + ((size_t)blockIdx.x * WPB + (threadIdx.x >> 6)) * (NS * NS) : nullptr);
    if (C.paramEstSetting == 2 && lane <= C.N) { predp[lane] = sp; predp[64 + lane] = vp; }
    codes[(size_t)b * 64 + lane] = shift_codes(code, C.N);
    write_out(out, 0, B, b, so, lane);
    if (s_pred && lane <= C.N) s_pred[(size_t)lane * B + b] = sp;
    if (v_pred && lane <= C.N) v_pred[(size_t)lane * B + b] = vp;
    if (lane == 0) { status[b] = so.status; if (iters) iters[b] = so.iters; }
}

// B1: closed loop over n_steps for B instances (ABO/RunOpt_ABMPC.m:154-340) in work units (run_units, eepacc_units.h).
// Ts and the LDS layout are fixed for the launch (Cp[0]); the settings are bound per work unit.  With classes, every C
// inside the unit's body is that binding (it shadows the kernel's class-0 C), est_preview's argument included.
// k_start > 0 resumes from the carried per-instance state (carry [6][B], see Carry; codes: shifted working set).  The
// small-horizon kernel is compiled for 2 waves per SIMD (1: 512 registers, no scratch; measured slower).
template <int MMAX, int NS, int WPB, class... Extra>
__global__ void __launch_bounds__(64 * WPB, ((NS <= 32 && WPB >= 4) ? 2 : 1))
k_run_abmpc(const DevCfg* __restrict__ Cp, int B, int k_start, int n_steps,
            const double* __restrict__ s0, const double* __restrict__ v0, const double* __restrict__ a_m1,
            const double* __restrict__ s_tv, const double* __restrict__ v_tv,
            double* __restrict__ carry, unsigned long long* __restrict__ codes,
            double* __restrict__ traj, int32_t* __restrict__ status, int32_t* __restrict__ iters_total,
            int* __restrict__ work_counter, int* __restrict__ done, int kChunkSteps,
            int* __restrict__ err_word, int spin_limit, Extra... extra) {
    extern __shared__ __align__(16) unsigned char smem[];
    const DevCfg& C = *Cp;                               // with classes: class 0, for what is fixed for the launch
    rc_table_init<MMAX>();
    double* Hs;
    WaveMem<MMAX, NS>& M = *wave_mem<MMAX, NS>(smem, C.N, Hs);
    const int lane = lane_id();
    const double Ts = C.Tvec[0];
#ifdef EEPACC_BL_TRACE
    if (B == 1) g_trace_on = 1;
#endif
    run_units(B, n_steps, kChunkSteps, work_counter, done, err_word, spin_limit, status, iters_total, [&](int b, int kk0, int kk1) {
        EEPACC_AB_UNIT_CFG
        unsigned long long code = 0ull;
        Carry cs;
        if (k_start + kk0 > 0) {
            cs.load(carry, B, b);
            code = codes[(size_t)b * 64 + lane];
        }
        int it_total = 0;
        double* predp = C.pred + (size_t)b * 128;
        for (int kk = kk0; kk < kk1; ++kk) {
            StepIn in;
            if constexpr (kTargetVeh) measure_no_lead(C, Ts, k_start + kk, b, s0, v0, a_m1, cs, in);
            else measure(C, Ts, k_start + kk, kk, B, b, s0, v0, a_m1, s_tv, v_tv, cs, in);
            StepOut so;
            double sp, vp;
            if constexpr (kEst)
                ab_step<MMAX, NS>(C, M, Hs, in, code, so, sp, vp, predp, kk > kk0, nullptr,
                                  est_preview(C, lane, B, b, kk, s_tv, v_tv, extra...));
            else
            ab_step<MMAX, NS>(C, M, Hs, in, code, so, sp, vp, predp, kk > kk0,
                              kIce ? C.hb + ((size_t)blockIdx.x * WPB + (threadIdx.x >> 6)) * (NS * NS) : nullptr);
            if (C.paramEstSetting == 2) {
                WSYNC();
                if (lane <= C.N) { M.ws[lane] = sp; M.wv[lane] = vp; }
                WSYNC();
                if (kk == kk1 - 1 && lane <= C.N) { predp[lane] = sp; predp[64 + lane] = vp; }
            }
            code = shift_codes(code, C.N);
            write_out(traj, (size_t)kk * EEPACC_OUT_N, B, b, so, lane);
            if (lane == 0) status[(size_t)kk * B + b] = so.status;
            it_total += so.iters;
            cs.advance(so, Ts);
        }
        codes[(size_t)b * 64 + lane] = code;
        if (lane == 0) cs.store(carry, B, b);
        return it_total;
    });
}

// the kernels of this instantiation as the host launches them: with the class map where the variant has one
template <int MMAX, int NS, int WPB> constexpr auto step_kernel() {
    if constexpr (kEst && kClasses) return &k_ab_step<MMAX, NS, WPB, const int32_t*, const double*, const double*, const double*>;   // class_of, then est's
    else if constexpr (kEst) return &k_ab_step<MMAX, NS, WPB, const double*, const double*, const double*>;      // s_est, v_est, s_tv_est
    else if constexpr (kClasses) return &k_ab_step<MMAX, NS, WPB, const int32_t*>;
    else return &k_ab_step<MMAX, NS, WPB>;
}
template <int MMAX, int NS, int WPB> constexpr auto run_kernel() {
    if constexpr (kEst && kClasses) return &k_run_abmpc<MMAX, NS, WPB, const int32_t*, const int32_t*, const double*, int>;   // class_of, then est's
    else if constexpr (kEst) return &k_run_abmpc<MMAX, NS, WPB, const int32_t*, const double*, int>;             // idx, frac, n_lead
    else if constexpr (kClasses) return &k_run_abmpc<MMAX, NS, WPB, const int32_t*>;
    else return &k_run_abmpc<MMAX, NS, WPB>;
}

}  // namespace EEPACC_IMPL_NS
}  // namespace eepacc
