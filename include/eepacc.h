/*
 * eepacc.h -- C ABI of libeepacc, the MI355X-native batched EEPACC MPC engine.
 *
 * Drop-in boundary for the per-step RunOpt_ABMPC / RunOpt_FBMPC hot path of
 * stefavpolito/EEPACC_MPC_CasADi_MATLAB.  Every entry point cites the
 * reference interface it replaces.  Paths: ABO/ = ACCMPC-ABO_CasADi/, ORIG/ = MATLAB_CasADi/.
 *
 * Conventions
 *   - plain C, plain pointers and sizes; no C++/torch types.
 *   - all floating point data is IEEE fp64 (the reference is MATLAB double throughout).
 *   - batched arrays are batch-major structure-of-arrays: x[k*B + i] is item k (a horizon
 *     stage or a simulation step) of instance i, unit stride across instances.
 *   - "device" pointers are HIP device allocations on the handle's GPU (e.g. a torch
 *     tensor's data_ptr()); "host" entry points end in _host and copy in/out themselves.
 *   - every function returns 0 on success or a negative EEPACC_E* code.  A QP that does not
 *     converge is NOT an error: like the reference (opts.error_on_fail=false,
 *     ABO/RunOpt_ABMPC.m:121,255) the iterate is still applied and status[i] = 1 mirrors
 *     optSol.exitMessage(k).
 *   - a handle owns its device workspaces and per-instance warm-start state; it is
 *     thread-compatible (one handle per host thread / stream), not thread-safe, and admits ONE
 *     launch in flight at a time: the closed-loop kernels hand their loop state from work unit to
 *     work unit through buffers of the handle, so a second eepacc_run_* on another stream of the
 *     same handle must wait for the first (use one handle per concurrent stream).
 *   - status values: 0 solved, 1 QP not converged / infeasible (the reference's exitMessage),
 *     3 the step was not computed because a device-side wait timed out (then eepacc_synchronize
 *     returns EEPACC_EDEVICE; never expected in normal operation).
 */
#ifndef EEPACC_H
#define EEPACC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EEPACC_VERSION 1

#define EEPACC_OK            0
#define EEPACC_EINVAL       -1   /* malformed argument / unsupported setting            */
#define EEPACC_ENOMEM       -2   /* host or device allocation failed                   */
#define EEPACC_EDEVICE      -3   /* HIP runtime error (message: eepacc_last_error())   */
#define EEPACC_ENOTSUP      -4   /* setting valid in the reference but not built here  */

#define EEPACC_MAX_HORIZON   63  /* N_hor upper limit of the HIP kernels               */
#define EEPACC_QP_MAX_NV    384  /* dense QP operator: variables                       */
#define EEPACC_QP_MAX_NC   2048  /* dense QP operator: rows of A                       */

/* Vehicle constants: the struct V returned by SetVehicleParameters()
 * (ABO/Functions/Settings/SetVehicleParameters.m:12-133; ORIG/ holds the BMW i3 values). */
typedef struct eepacc_vehicle {
    double m, A_f, c_d, L, h_g, WD_s_F, L_f, L_r;
    double F0, F1, F2;             /* coast-down (ABO only)                             */
    double p00, p10, p01;          /* efficiency-map fit used by the fuel term (ABO)    */
    double P_m_max, T_m_max, omega_m_r, omega_m_max;
    double c_r, R_w, beta_gb, beta_fd, phi;
    double v_max;
    double eta_TF;
    double lambda, mu, rho_a, g, zeta_a;
    /* ICE fuel-map fit FC = k00 + k10*w_ICE + k01*T_ICE and the stepped gearbox it needs
     * (ABO/Functions/Settings/SetVehicleParameters.m:44-46,96-101; gear choice per horizon stage:
     * ABO/Functions/MPCs/LUTgearshift.m:17-41).  Read only when ab_fuel_term = 2. */
    double k00, k10, k01;
    double tau_fd, eta_drive;
    double upSpd[7];               /* upshift speed thresholds, m/s, ascending          */
    double tau_gb[8];              /* gearbox ratio of gears 1..8                       */
} eepacc_vehicle;

/* Controller / scenario settings: the fields of OPTsettings read on the hot path
 * (ABO/Settings.m, ABO/Functions/Settings/GenerateUseCase.m). */
typedef struct eepacc_settings {
    /* horizon (ABO/Settings.m:101-122, 243-250) */
    int32_t N_hor;
    const double*  Tvec;           /* [N_hor]  Tvec[0] is the controller sample time Ts */
    const int32_t* Mb;             /* [N_hor]  move-blocking mask, may be NULL (= zeros) */
    /* weights.  W_AB: ABO/Settings.m:48-64 has 7 entries [w_FC,w_a,w_j,w_v,w_h,w_s,w_f];
     * ORIG/Settings.m:48-62 has 6 (no w_FC): set ab_fuel_term = 0 and pass
     * [0,w_a,w_j,w_v,w_h,w_s,w_f].  W_FB: ABO/Settings.m:31-46 [w_P,w_a,w_j,w_v,w_h,w_s,w_f] */
    double  W_AB[7];
    double  W_FB[7];
    int32_t ab_fuel_term;          /* 1: efficiency-map fuel term ABO/.../CreateQP_AB.m:162-166;
                                    * 2: the ICE-map fuel term of :154-159 (what savedABMPCsolICEMAP.mat was
                                    *    written with): per-stage curvature 2 w_FC k01 F2 R_w/(tau_fd tau_est(k) eta_drive)
                                    *    with the gear ratio tau_est(k) = LUTgearshift(v_est(k)), so H changes every
                                    *    step; 0: no fuel term (ORIG)                                               */
    int32_t ab_route_rows;         /* 1: ORIG 18-row stage (speed/curve/stop/TL caps)    */
    /* vehicle following (ABO/Settings.m:203-204,143) */
    double  tau_min, h_min, s_goal;
    /* estimators (ABO/Settings.m:105-108) */
    int32_t paramEstSetting, TVestSetting;
    double  tConstACC_ego, tConstACC_tar;
    /* plant (ABO/Settings.m:111) */
    int32_t N_integratePlant;
    /* solver selection (ABO/Settings.m:98,114): 0 and 1 (sparse / dense qpOASES) pose the same QP and
     * are both accepted; 2 (HPIPM formulation with hard acceleration bounds) is not built */
    int32_t solverToUse;
    int32_t FBuseTaylor;
    /* power fits (ABO/Settings.m:229-238) */
    double  b_quadr[6];
    double  b_fifthOrder[21];
    /* route tables produced by GenerateUseCase (piecewise tables, knots ascending) */
    int32_t n_speedLim;  const double* s_speedLim;  const double* v_speedLim;
    int32_t n_curv;      const double* s_curv;      const double* curvature;
    int32_t n_slope;     const double* s_slope;     const double* slope;
    int32_t n_stop;      const double* stopLoc;
    int32_t n_TL;        const double* TLLoc;      /* [n_TL][4] row-major: loc,phase,red,green */
    double  stopRefDist, stopRefVelSlope, stopVel, TLstopVel, TLStopRegionSize, alpha_TTL;
    /* Baseline controller (ABO/RunOpt_BLMPC.m, ABO/Functions/MPCs/CreateQP_BL.m).  bl_mode = 1 makes a handle
     * a RunOpt_BLMPC: the ABMPC entry points (eepacc_ab_step, eepacc_run_abmpc, ...) then pose CreateQP_BL's problem
     * (n_u = 2: a, xi_f; one slack for all soft rows; objective -w_v sum v_k + w_a a^2 + w_j jerk^2 + w_f xi_f) with
     * the baseline comfort limits of EstimateRouteAndComfortBounds.m:173-189 (MPCtype 1).  The caller passes
     * N_hor = BL_N_hor, Tvec[k] = BL_Ts and paramEstSetting = BL_trajEstSett (ABO/Settings.m:137-139,
     * EstimateVehicleTrajectory.m:25-29); W_AB / W_FB are ignored.  W_BL = [w_v, w_a, w_j, w_f] (ABO/Settings.m:66-71).
     * With the reference's weights (w_a = w_j = 0) the problem is a linear program; the dual active set needs curvature,
     * so it is solved by the proximal-point iteration  a_{j+1} = argmin LP(a) + bl_lp_eps/2 |a - a_j|^2,  a_0 = 0
     * (bl_lp_eps <= 0: 0.1), each solve warm from the last working set, until the point stays (at most bl_prox_iter
     * re-centrings; 0: 40, < 0: none, i.e. the single regularised solve of earlier versions): for a linear program that
     * ends after finitely many steps at an optimum of the LP itself.
     *
     * Target-vehicle MPC (ABO/RunOpt_TVMPC.m, ABO/Functions/MPCs/CreateQP_TV.m).  bl_mode = 2 makes a handle a
     * RunOpt_TVMPC, the controller that synthesises a lead vehicle's trace along the route.  It poses CreateQP_TV's
     * problem (solverToUse 0 / 1 branch, z = [s v a xi_f]): CreateQP_BL's without the two headway rows per stage and the
     * two rows of the terminal stage, with 0.8 of the speed-limit and curve caps (:262-272; stop and traffic-light caps
     * unscaled) and the comfort limits evaluated at v_est = 0 (:44-45), i.e. the low-speed limits at every stage.  The
     * struct has no fields of its own for it; the caller passes N_hor = TV_N_hor, Tvec[k] = TV_Ts (uniform; it is also
     * the plant's step, RunPlantModel.m steps Tvec(1), so TV_Ts must equal the ego controller's Tvec(1)),
     * paramEstSetting = TV_trajEstSett, W_BL = W_TV = [w_v, w_a, w_j, w_f] and BL_a_LimLowVel .. BL_j_LimHighVel =
     * TV_a_LimLowVel .. TV_j_LimHighVel (ABO/Settings.m:73-78,207-218); bl_lp_eps / bl_prox_iter act as for bl_mode = 1
     * (W_TV is a linear program too).  tau_min, h_min, TVestSetting and tConstACC_tar are not read.  Such a handle runs
     * through eepacc_tv_step / eepacc_run_tvmpc / eepacc_run_tvmpc_host only; every ABMPC / BLMPC / FBMPC entry point
     * returns EEPACC_EINVAL on it.  solverToUse = 2 (n_x = 3, hard +-8 m/s^2 bounds) stays EEPACC_ENOTSUP. */
    int32_t bl_mode, bl_prox_iter;
    double  W_BL[4];
    double  BL_a_LimLowVel, BL_a_LimHighVel, BL_j_LimLowVel, BL_j_LimHighVel;   /* ABO/Settings.m:131-134 */
    double  bl_lp_eps;
    /* ABMPC / baseline controller: a measured state that violates its own hard bounds (s_0 >= 0, 0 <= v_0 <= v_max,
     * CreateQP_AB.m:256-261, CreateQP_BL.m:214-222) by more than this makes the step infeasible (status 1).
     * <= 0: 1e-9 (baseline controller: 1e-5 m/s), which lets the closed loop's rounding noise at standstill through (the
     * saved ABMPC solutions have exitMessage = 0 there); 1e-11 reproduces the three bad exits of the saved baseline
     * solution (v_0 = -3e-10). */
    double  state_bound_tol;
} eepacc_settings;

typedef struct eepacc_handle eepacc_handle;

/* Number of doubles per instance in the per-step output block, batch-major [EEPACC_OUT_N][B]. */
enum {
    EEPACC_OUT_S = 0,     /* s_opt(k)   = z(1)  measured position the QP was solved at      */
    EEPACC_OUT_V,         /* v_opt(k)   = z(2)                                              */
    EEPACC_OUT_FM,        /* Fm_opt(k)  motor force after allocation (AB) / QP output (FB)  */
    EEPACC_OUT_FB,        /* Fb_opt(k)                                                      */
    EEPACC_OUT_A,         /* a_opt(k)   realised acceleration (ABO/RunOpt_ABMPC.m:324)      */
    EEPACC_OUT_XI_V, EEPACC_OUT_XI_H, EEPACC_OUT_XI_S, EEPACC_OUT_XI_F,
    EEPACC_OUT_COST,      /* sol.cost (dense-QP objective value, constant term excluded)    */
    EEPACC_OUT_DISTHOR,   /* DistHor(k) (ABO/RunOpt_ABMPC.m:200)                            */
    EEPACC_OUT_AQP,       /* QP stage-0 acceleration before allocation (z(3), AB only)      */
    EEPACC_OUT_N
};

const char* eepacc_last_error(void);
int  eepacc_version(void);
int  eepacc_sizeof_settings(void);   /* sizeof(eepacc_settings) as compiled: binding self-check */
int  eepacc_sizeof_vehicle(void);

/* Create / destroy.  Replaces the one-time set-up part of RunOpt_ABMPC / RunOpt_FBMPC
 * (ABO/RunOpt_ABMPC.m:14-123: unpack settings, state-space matrices, conic(...) creation).
 * device: HIP device ordinal.  max_batch: largest B used with this handle. */
int  eepacc_create(eepacc_handle** out, const eepacc_settings* S, const eepacc_vehicle* V,
                   int device, int max_batch);
void eepacc_destroy(eepacc_handle* h);

/* Settings classes: one handle for instances that differ in route, weights, estimator or vehicle, ABMPC only.  The
 * reference runs one OPTsettings per call (ABO/Main.m:44-99, one useCaseNum of ABO/Functions/Settings/GetUseCase.m or one
 * point of a Settings.m sweep at a time); here S[n_classes], V[n_classes] hold the settings and the vehicle of every class
 * and each instance of a launch belongs to one of them, so the twelve use cases or a sweep over W_AB or the vehicle mass
 * run in one launch.  Every class is validated like the settings of eepacc_create, before the device is touched.  What
 * selects the kernel and the launch geometry must agree: N_hor and every entry of Tvec equal those of class 0
 * (EEPACC_EINVAL otherwise), and no class may have move blocking (Mb all zero or NULL), ab_fuel_term = 2 or bl_mode != 0
 * (EEPACC_ENOTSUP; eepacc_create_classes_bl below takes the classes of the baseline and target-vehicle controllers); the
 * message names the class and the field.  Everything else may differ per class: the route tables,
 * ab_route_rows, ab_fuel_term 0 or 1, W_AB, tau_min, h_min, s_goal, the estimator modes and time constants,
 * N_integratePlant, state_bound_tol, b_fifthOrder and the whole vehicle.  n_classes must be in [1, EEPACC_MAX_CLASSES].
 *
 * Such a handle runs eepacc_ab_step, eepacc_run_abmpc (also resumed in chunks), eepacc_run_abmpc_host and
 * eepacc_postprocess (each instance with the settings of its class) and eepacc_reset, eepacc_synchronize,
 * eepacc_last_iterations; the FBMPC, BLMPC, TVMPC and dense-QP entry points return EEPACC_ENOTSUP on it.  FBMPC on its
 * classes (each settings struct carries W_FB, FBuseTaylor and b_quadr) has entries of its own, eepacc_classes_fb_step and
 * eepacc_run_classes_fbmpc, after eepacc_run_fbmpc; eepacc_fb_step / eepacc_run_fbmpc keep refusing the handle.  It runs the
 * class kernels also with n_classes = 1; the results of an instance are bit for bit those of a handle created by
 * eepacc_create from the settings of its class. */
#define EEPACC_MAX_CLASSES 4096
int  eepacc_create_classes(eepacc_handle** out, const eepacc_settings* S, const eepacc_vehicle* V,
                           int n_classes, int device, int max_batch);

/* Settings classes for the baseline controller (bl_mode = 1, RunOpt_BLMPC) and the target-vehicle controller (bl_mode = 2,
 * RunOpt_TVMPC): the yardstick of the twelve use cases in one BLMPC launch, and a lead vehicle per route (ABO/Main.m:82-89)
 * in one TVMPC launch.  eepacc_create_classes keeps refusing bl_mode != 0; this entry takes those classes.  Every class is
 * validated like the settings of eepacc_create before the device is touched, the message naming the class and the field.
 * bl_mode of class 0 must be 1 or 2 (0: EEPACC_EINVAL, use eepacc_create_classes) and every class must have class 0's
 * bl_mode, N_hor and Tvec (EEPACC_EINVAL otherwise); n_classes must be in [1, EEPACC_MAX_CLASSES].  Everything else may
 * differ per class: the route tables, W_BL, BL_a_Lim*, BL_j_Lim*, bl_lp_eps, bl_prox_iter, tau_min, h_min, s_goal,
 * paramEstSetting, TVestSetting and the time constants, N_integratePlant, state_bound_tol, b_fifthOrder and the whole
 * vehicle.
 *
 * A handle with bl_mode = 1 runs eepacc_ab_step / eepacc_bl_step, eepacc_run_abmpc / eepacc_run_blmpc (also resumed in
 * chunks) and their _host forms; one with bl_mode = 2 runs eepacc_tv_step, eepacc_run_tvmpc and eepacc_run_tvmpc_host.  Both
 * run eepacc_postprocess, eepacc_kpis, eepacc_follow_kpis, eepacc_route_kpis (each instance with the tables of its class),
 * eepacc_set_classes, eepacc_num_classes, eepacc_reset, eepacc_synchronize and eepacc_last_iterations, and a launch needs
 * the class map of its B as on a handle of eepacc_create_classes.  The results of an instance are bit for bit those of a
 * handle created by eepacc_create from the settings of its class.
 *
 * Refused with EEPACC_ENOTSUP: FBMPC, the dense QP operator, every _qp_size / _qp_rows / _build_qp, the _est entries and
 * the two _preview loops.  A bl_mode = 2 handle on an ABMPC / BLMPC entry and a bl_mode = 1 handle on a TVMPC entry answer
 * EEPACC_EINVAL, as the handles of eepacc_create with those modes do.  A handle of eepacc_create_classes (ABMPC classes)
 * on eepacc_bl_* / eepacc_tv_* stays EEPACC_ENOTSUP. */
int  eepacc_create_classes_bl(eepacc_handle** out, const eepacc_settings* S, const eepacc_vehicle* V,
                              int n_classes, int device, int max_batch);

/* class_of_host [B], host, values in [0, n_classes): the class of instance i in the launches that follow.  The map is
 * copied to the device (after waiting for the device's pending work) and the carried loop state is reset like
 * eepacc_reset, since a change of the map in mid-simulation has no meaning.  B > max_batch or a value out of range:
 * EEPACC_EINVAL, and the previous map stays.  A launch on a handle of eepacc_create_classes whose B differs from the last
 * eepacc_set_classes, or with none made, returns EEPACC_EINVAL.  eepacc_reset keeps the map. */
int  eepacc_set_classes(eepacc_handle* h, int B, const int32_t* class_of_host);

/* Number of settings classes of a handle; 1 for a handle from eepacc_create. */
int  eepacc_num_classes(const eepacc_handle* h);

/* Reset the per-instance carried state (warm start, previous lead speed, FB A/D freeze,
 * step counter): the "kk == 0" branch of ABO/RunOpt_ABMPC.m:159-172. */
int  eepacc_reset(eepacc_handle* h);

/* B2 -- per-step operator: one receding-horizon step of ABMPC for B instances
 * (body of the kk-loop ABO/RunOpt_ABMPC.m:193-329 after the measurement block, the estimators :193-200 included: the
 * horizon guesses are computed from the measured state and lead sample by the handle's paramEstSetting / TVestSetting.
 * The Simulink MATLAB-Function block ACCMPC(N_hor, Tvec, s_measured, v_measured, s_est, v_est, s_tv_est, OPTsettings, V)
 * of ABO/ACCMPC.slx chart_121 takes those guesses as inputs: that contract is eepacc_ab_step_est's, below).
 * Inputs, device, each [B]: s, v (measured state), a_prev (a_minus1), t0, s_tv, v_tv,
 * a_tv_prev (lead acceleration estimate).  Outputs, device: out[EEPACC_OUT_N][B];
 * s_pred,v_pred [(N_hor+1)][B] = z(1:7:end), z(2:7:end) (may be NULL); status [B] int32.
 * stream: hipStream_t as void* (NULL = default stream).  Asynchronous on that stream. */
int  eepacc_ab_step(eepacc_handle* h, int B,
                    const double* s, const double* v, const double* a_prev, const double* t0,
                    const double* s_tv, const double* v_tv, const double* a_tv_prev,
                    double* out, double* s_pred, double* v_pred, int32_t* status,
                    void* stream);

/* The same step with the horizon guesses supplied: the contract of the Simulink block ACCMPC(..., s_est, v_est, s_tv_est, ...)
 * and of CreateQP_AB(OPTsettings, n_x, n_u, s_0, v_0, s_est, v_est, s_tv_est, t_0, a_minus1) (ABO/RunInit_ABMPC.m:58,
 * RunOpt_ABMPC.m:204), for a lead prediction of the caller's own (a communicated plan, a learned predictor, a tracker).
 * s_est, v_est, s_tv_est: device arrays [N_hor+1][B], as EstimateVehicleTrajectory returns them (the layout of s_pred / v_pred,
 * so a prediction output can be fed back in).  s_est and v_est are given together or both NULL; NULL: the handle's
 * paramEstSetting.  s_tv_est may be NULL: the handle's TVestSetting.  Row N_hor of s_tv_est is not read (the terminal rows
 * use s_tv_est(N), CreateQP_AB.m:376-387).  Row 0 of s_est and v_est is used as given (the reference passes the measurement
 * there) and is not overwritten.  +inf in s_tv_est: no lead at that stage.  With all three NULL the entries compute what
 * eepacc_ab_step / eepacc_ab_build_qp compute.  Every other argument as in eepacc_ab_step / eepacc_ab_build_qp.
 * eepacc_ab_step_est reads and writes exactly the handle state eepacc_ab_step does (warm start, carried predictions,
 * iteration counts): the two can alternate on one handle.  eepacc_ab_build_qp_est reads no solver state and writes none;
 * eepacc_ab_qp_size and eepacc_ab_qp_rows describe its output.  s_tv_est enters the problem only through uba of the rows
 * EEPACC_AB_ROW_SAFE1, _SAFE2 and _HWP, so the derivative of the solution with respect to the lead prediction is one adjoint
 * solve on the built problem (qp_sens.ab_lead_gradient of the Python package).
 *
 * eepacc_run_abmpc_preview: eepacc_run_abmpc with the lead's horizon guess read from the lead trace itself (perfect preview);
 * the ego estimator stays the handle's.  s_tv, v_tv [n_lead][B], n_lead >= n_steps: rows 0 .. n_steps-1 are the measurements
 * of this launch's steps as in eepacc_run_abmpc (resumed launches pass the continued rows), the rows after them the future
 * that the last steps look into.  At the step of row r, stage k lies tau_k = sum_{i<k} Tvec[i] ahead, at row r + p with
 * p = tau_k / Tvec[0]; idx = floor(p) and frac = p - idx are computed once per handle in long double, frac snapped to 0 below
 * 1e-9 and to the next index above 1 - 1e-9.  The guess is the sample s_tv[r+idx] where frac = 0 (no arithmetic), else
 * (1-frac) s_tv[r+idx] + frac s_tv[r+idx+1], and past the last row s_tv[n_lead-1] + v_tv[n_lead-1] (t - t_last).  A lead at
 * +inf (no lead, Main.m:77-80) stays +inf.  scenarios.lead_preview of the Python package states the rule in numpy.
 *
 * EEPACC_ENOTSUP, the message naming the cause: a handle of eepacc_create_classes / _classes_bl, bl_mode != 0, any Mb[k] != 0,
 * ab_fuel_term == 2.  EEPACC_EINVAL: a NULL required buffer, s_est without v_est or the reverse, B out of range,
 * n_lead < n_steps.  B = 0 returns EEPACC_OK.
 * The baseline controller's counterparts are eepacc_bl_step_est, eepacc_bl_build_qp_est and eepacc_run_blmpc_preview, below; on a
 * bl_mode = 1 handle the message of these three entries points to them.
 * Class handles have entries of their own, eepacc_classes_step_est and eepacc_run_classes_preview, below.
 * FBMPC's counterparts are eepacc_fb_step_est, eepacc_fb_build_qp_est and eepacc_run_fbmpc_preview, after eepacc_fb_build_qp.
 * Not built: supplied guesses for FBMPC steps through the dense path (the builder entry serves such handles) and for FBMPC
 * settings classes, for the target-vehicle controller, for move blocking and the ICE map, and a preview of the ego estimate.
 * Cost against eepacc_ab_step / eepacc_run_abmpc: tools/gpu_ab_est_bench.py, DESIGN.md section 3.4f. */
int  eepacc_ab_step_est(eepacc_handle* h, int B,
                        const double* s, const double* v, const double* a_prev, const double* t0,
                        const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        const double* s_est, const double* v_est, const double* s_tv_est,
                        double* out, double* s_pred, double* v_pred, int32_t* status, void* stream);
int  eepacc_ab_build_qp_est(eepacc_handle* h, int B,
                            const double* s, const double* v, const double* a_prev, const double* t0,
                            const double* s_tv, const double* v_tv, const double* a_tv_prev,
                            const double* s_est, const double* v_est, const double* s_tv_est,
                            double* H, double* g, double* A, double* lba, double* uba, void* stream);
int  eepacc_run_abmpc_preview(eepacc_handle* h, int B, int n_steps, int n_lead,
                              const double* s0, const double* v0, const double* a_minus1,
                              const double* s_tv, const double* v_tv,
                              double* traj, int32_t* status, void* stream);

/* B1 -- closed loop: optSol = RunOpt_ABMPC(OPTsettings) for B independent instances
 * (ABO/RunOpt_ABMPC.m:154-340 incl. measurement block, plant, force allocation).
 * n_steps = N_sim+1 iterations (kk = 0..N_sim).  Device inputs: s0,v0,a_minus1 [B];
 * s_tv,v_tv [n_steps][B] lead traces (already shifted by TVlength, ABO/Main.m:88).
 * Device outputs: traj [n_steps][EEPACC_OUT_N][B]; status [n_steps][B].
 * The handle carries the loop state: the first call after eepacc_create/eepacc_reset starts
 * at kk = 0, later calls continue where the previous one stopped (s_tv/v_tv then hold the
 * rows of the continued steps), so a long simulation can be run in chunks. */
int  eepacc_run_abmpc(eepacc_handle* h, int B, int n_steps,
                      const double* s0, const double* v0, const double* a_minus1,
                      const double* s_tv, const double* v_tv,
                      double* traj, int32_t* status, void* stream);

/* The condensed QP of one ABMPC step as data: what a user of the reference holds in the workspace as H, c, G, g_lb, g_ub
 * (ABO/RunOpt_ABMPC.m:238-252, solverToUse = 1) and finds saved as optSol.H, optSol.G.  The ABMPC kernels above never form it;
 * eepacc_ab_build_qp does, for the inputs of eepacc_ab_step (device, each [B]): the estimators and bounds
 * (EstimateVehicleTrajectory.m:55-88, EstimateRouteAndComfortBounds.m:63-171), the objective and rows of
 * ABO/Functions/MPCs/CreateQP_AB.m:150-387 with the zero rows trimmed as RunOpt_ABMPC.m:229-233 does, condensed as
 * TransformToDenseFormulation.m:30-91.  Outputs, device, instance-major, in the layout eepacc_qp_solve_batched reads:
 * H [B][nV*nV], g [B][nV], A [B][nV][nC] (column-major nC x nV), lba, uba [B][nC], an absent side -inf / +inf.  There are no
 * lbx / ubx: the reference passes infinite ones in the dense branch (:100-104); hand the operator NULL.
 * nV = 5 N_hor, variables per stage a, xi_v, xi_h, xi_s, xi_f.  nC = 14 N_hor + 2 (ABO) or 18 N_hor + 2 (ab_route_rows = 1)
 * plus one row per blocked stage (Mb[k] = 1, CreateQP_AB.m:283-289), rows in the reference's order; eepacc_ab_qp_size
 * returns both.  Covered: both trees, ab_fuel_term 0, 1 and 2, Mb, variable Tvec, every N_hor the handle accepts, the
 * estimator modes 0, 1 and 2 (mode 2 reads the predictions the handle carries from the last step and does not write them).
 *
 * eepacc_ab_qp_rows fills two host arrays [nC]: stage[i] in 0 .. N_hor-1, or N_hor for the two terminal rows
 * (CreateQP_AB.m:376-387), and type[i], one of EEPACC_AB_ROW_*, so that lam_a and ws_a of eepacc_qp_solve_batched_dual on
 * the built problem can be read row by row.  The values ascend in the order of the rows within a stage: */
enum {
    EEPACC_AB_ROW_S = 0,     /* CreateQP_AB.m:256-279  0 <= s_k <= s_goal                                                  */
    EEPACC_AB_ROW_V,         /*   0 <= v_k <= v_max                                                                        */
    EEPACC_AB_ROW_XI_V,      /*   xi_v >= 0                                                                                */
    EEPACC_AB_ROW_XI_H,      /*   xi_h >= 0                                                                                */
    EEPACC_AB_ROW_XI_S,      /*   xi_s >= 0                                                                                */
    EEPACC_AB_ROW_XI_F,      /*   xi_f >= 0                                                                                */
    EEPACC_AB_ROW_BLOCKED,   /* :283-289  a_{k-1} - a_k = 0, only on a stage with Mb[k] = 1                                */
    EEPACC_AB_ROW_A_MAX,     /* :292-299  a_k - xi_f <= a_max                                                              */
    EEPACC_AB_ROW_A_MIN,     /*   a_k + xi_f >= a_min                                                                      */
    EEPACC_AB_ROW_J_MAX,     /* :302-322  a_k - a_{k-1} - xi_f <= T_k j_max (stage 0: a_minus1 on the right-hand side)     */
    EEPACC_AB_ROW_J_MIN,     /*   a_k - a_{k-1} + xi_f >= T_k j_min                                                        */
    EEPACC_AB_ROW_V_LIM,     /* ORIG/.../CreateQP_AB.m:307-329, only with ab_route_rows:  v_k - xi_f <= speed limit        */
    EEPACC_AB_ROW_V_CURV,    /*   v_k - xi_f <= curve speed                                                                */
    EEPACC_AB_ROW_V_STOP,    /*   v_k - xi_s <= stop speed                                                                 */
    EEPACC_AB_ROW_V_TL,      /*   v_k - xi_s <= traffic-light speed                                                        */
    EEPACC_AB_ROW_V_INC,     /* :349-352  speed incentive  v_k + xi_v >= min(speed limit, curve speed)                     */
    EEPACC_AB_ROW_SAFE1,     /* :355-362  safe distance 1  s_k - xi_s <= s_tv - h_min (terminal row: no slack)             */
    EEPACC_AB_ROW_SAFE2,     /*   safe distance 2  s_k + tau_min v_k - xi_s <= s_tv (terminal row: no slack)               */
    EEPACC_AB_ROW_HWP,       /* :365-371  headway policy  s_k + (T_hwp + G_hwp v_est) v_k - xi_h <= s_tv - A_hwp           */
    EEPACC_AB_ROW_N
};
/* The built problem is the reference's own.  A measured state outside its hard bounds shows up as a stage-0 row without
 * coefficients whose bounds exclude 0 (the operator then reports status 1); the tolerance state_bound_tol of the ABMPC
 * kernels is not applied.  The constant term of the objective is excluded: 1/2 x'Hx + g'x at the solution equals
 * EEPACC_OUT_COST of the same step, x[0] is EEPACC_OUT_AQP and x[1..4] are the four slack outputs.
 *
 * The build is asynchronous on stream.  It reads no solver state of the handle (warm start, loop counters, carry) and writes
 * none: a build between two ABMPC calls leaves their results bit for bit unchanged.  One workgroup per instance writes every
 * entry, zeros included (no memset, no atomics): the arrays do not depend on B or on timing.  EEPACC_EINVAL, with a message
 * that names the argument: a NULL buffer, B < 0 or B > max_batch.  EEPACC_ENOTSUP: a handle of eepacc_create_classes (nC can
 * differ per class) and a handle created with bl_mode 1 or 2, whose problem eepacc_bl_build_qp builds.  B = 0 returns
 * EEPACC_OK.
 * The FBMPC problem: eepacc_fb_build_qp below; the BLMPC and TVMPC problems: eepacc_bl_build_qp below.  Not built: class
 * handles, the formulations of solverToUse 0 (dynamics kept as rows) and 2 (HPIPM).
 * Throughput (tools/gpu_qp_build_bench.py --family ab, the build against a plain device fill of the same bytes,
 * profiles/ab_build_bench.json): 1.53 of the fill's time at N_hor = 20 x 4096 instances, 1.80 at N_hor = 60 x 1024; DESIGN.md
 * section 3.6a. */
int  eepacc_ab_qp_size(const eepacc_handle* h, int* nV, int* nC);
int  eepacc_ab_qp_rows(const eepacc_handle* h, int32_t* stage, int32_t* type);
int  eepacc_ab_build_qp(eepacc_handle* h, int B,
                        const double* s, const double* v, const double* a_prev, const double* t0,
                        const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        double* H, double* g, double* A, double* lba, double* uba, void* stream);

/* B3 -- dense QP operator: the call
 *   sol = QPsolver('h',H,'g',c,'a',G,'lbx',z_lb,'ubx',z_ub,'lba',g_lb,'uba',g_ub)
 * of ABO/RunOpt_ABMPC.m:252 and ABO/RunOpt_FBMPC.m:278 (CasADi conic, CAS/+casadi/conic.m:951-966)
 * for B independent problems of one shape:  min 1/2 x'Hx + g'x  s.t. lba <= Ax <= uba,
 * lbx <= x <= ubx.  Device arrays, instance-major: H [B][nV*nV] (symmetrised internally, so
 * row- or column-major), g [B][nV], A [B][nV][nC] = COLUMN-major nC x nV as MATLAB/CasADi hold
 * it, lba/uba [B][nC], lbx/ubx [B][nV]; +-inf entries and NULL bound arrays mean "absent".
 * x0 [B][nV] or NULL: proximal centre / initial guess (the reference passes none for AB and
 * hot-starts implicitly).  Outputs x [B][nV], cost [B] (may be NULL), status [B] (may be
 * NULL; 0 = KKT point verified, 1 = not converged).  H may be singular PSD or indefinite
 * (FB): a proximal term is added internally and removed by the final exact KKT solve. */
int  eepacc_qp_solve_batched(eepacc_handle* h, int B, int nV, int nC,
                             const double* H, const double* g, const double* A,
                             const double* lba, const double* uba,
                             const double* lbx, const double* ubx, const double* x0,
                             double* x, double* cost, int32_t* status, void* stream);

/* The same operator with the remaining outputs of the conic call (lam_a, lam_x: CAS/include/casadi/core/conic.hpp:199-208),
 * the final working set, and a warm start from one.  Layout, bound conventions, limits and refusals as above; x, cost and
 * status are those of eepacc_qp_solve_batched on the same inputs when no warm start is given.
 * lam_a [B][nC], lam_x [B][nV] (each may be NULL), CasADi's sign:  Hs x + g + A' lam_a + lam_x = 0 with Hs = (H+H')/2,
 * lam <= 0 where the lower side holds, lam >= 0 where the upper side holds, exactly 0.0 outside the final working set.
 * They are the multipliers of the verified KKT solve that accepted x; one that the verification let pass on the wrong
 * side of zero (by less than 1e-9 relative) is returned as 0.
 * ws_a [B][nC], ws_x [B][nV] (each may be NULL): -1 lower side in the final working set, +1 upper side, 0 neither; an
 * equality (lb == ub) shows the side the solver holds.  Where status != 0: lam_* are NaN and ws_* are 0.  Where the
 * proximal iteration ended by standing still (status 0 without a verified solve; x is the proximal point, feasible to
 * the iteration's tolerance), the multipliers come from one more exact solve on the working set.  They are stationary
 * and of the right sign to 1e-9 AT THAT SOLVE'S POINT, which is not the returned x and need not coincide with it: that
 * solve had just missed acceptance in the same round.  They are NaN (status stays 0, ws_* still name the working set)
 * if the system is singular or its multipliers miss stationarity or sign at 1e-9.  x and status are unaffected.
 * ws0_a [B][nC], ws0_x [B][nV], each may be NULL (both NULL, or all entries 0 for an instance: cold start): the sides
 * to start from, coded like ws_*.  Ignored per entry: any other value, a side without a finite bound, rows that depend
 * on the ones before them, everything beyond nV installed rows.  The set is kept only if all its multipliers are
 * non-negative for this problem, otherwise the solve starts cold; iteration, exact solve and verification are those of
 * the cold solve, so a status 0 means the same with and without a warm start.  There is no second attempt: a kept set
 * that is badly conditioned (dependence is refused only at 1e-14) can end an instance with status 1 that a cold solve
 * verifies -- a caller who needs the cold solve's status repeats the instances with status != 0 without ws0.
 * iters [B] (device, may be NULL): working-set iterations of the solve.  eepacc_last_iterations is not updated by this
 * entry point: it keeps the figures of the last call that wrote them. */
int  eepacc_qp_solve_batched_dual(eepacc_handle* h, int B, int nV, int nC,
                                  const double* H, const double* g, const double* A,
                                  const double* lba, const double* uba,
                                  const double* lbx, const double* ubx, const double* x0,
                                  const int8_t* ws0_a, const int8_t* ws0_x,
                                  double* x, double* cost, int32_t* status,
                                  double* lam_a, double* lam_x, int8_t* ws_a, int8_t* ws_x,
                                  int32_t* iters, void* stream);

/* Linear solves with the KKT matrix of a given working set: how the solution of the QP above moves with its data.
 * Per instance, with Hs = (H+H')/2, the rows i with ws_a[i] = +-1 and the variables j with ws_x[j] = +-1 held (any other
 * code: not held; the side does not enter; no bound is read), for each of nR >= 1 right-hand sides:
 *     Hs p + A_W' q_a + E_W' q_x = r_p                 (nV rows)
 *     A_i p = r_a[i]   on held rows,   p_j = r_x[j]   on held variables,   q_a[i] = q_x[j] = 0.0 elsewhere.
 * This is the system in CasADi's sign (Hs x + g + A'lam_a + lam_x = 0), where a row's multiplier is one signed number.
 * H, A as above; ws_a [B][nC], ws_x [B][nV] as the dual entry writes them (either may be NULL: none held);
 * r_p [B][nR][nV], r_a [B][nR][nC], r_x [B][nR][nV] (r_a, r_x may be NULL: zeros; entries outside the working set are
 * not read); outputs p, q_a, q_x of the same shapes (q_a, q_x may be NULL), status [B] (may be NULL).  The matrix is
 * factorised once per instance (single-non-zero rows eliminated, LU with partial pivoting) and every right-hand side is
 * refined twice against residuals evaluated from Hs and A.  More than nV held entries, or a smallest pivot below 1e-13
 * (dependent rows, Hs singular on their null space): status 1 and NaN in every output of that instance; the other
 * instances are unaffected.  Sizes, limits and refusals as for the operator above; nR < 1 is EEPACC_EINVAL.
 * Meaning.  With (x, lam_a, lam_x, ws_a, ws_x) from the dual entry, the solution on the FIXED working set is a linear
 * map of the data: the derivative below is the derivative of the QP's solution where the working set does not change
 * (strict complementarity), and the one-sided derivative on that set where a held row has lam == 0.
 *   Forward (directional derivative; d(.) are the data's directions, dHs = (dH+dH')/2):
 *     r_p = -(dg + dHs x + dA' lam_a),  r_a = d(bound of the held side) - dA x,  r_x = d(bound of the held side)
 *     gives p = dx, q_a = dlam_a, q_x = dlam_x.
 *   Adjoint (the matrix is symmetric; gx, glam_a, glam_x are the gradients of a scalar loss L):
 *     r_p = gx, r_a = glam_a, r_x = glam_x  gives (u, w_a, w_x) and
 *     dL/dg = -u;  dL/d(bound) = w on the side held, 0 elsewhere;  dL/dH = -(u x' + x u')/2;
 *     dL/dA = -(lam_a u' + w_a x')   (nC x nV). */
int  eepacc_qp_kkt_solve_batched(eepacc_handle* h, int B, int nV, int nC, int nR,
                                 const double* H, const double* A,
                                 const int8_t* ws_a, const int8_t* ws_x,
                                 const double* r_p, const double* r_a, const double* r_x,
                                 double* p, double* q_a, double* q_x,
                                 int32_t* status, void* stream);

/* Same two operators for the force-based MPC (ABO/RunOpt_FBMPC.m:161-331).  v_prev, Fm_prev,
 * Fb_prev are the previous step's state/controls (ABO/RunOpt_FBMPC.m:188-191). */
int  eepacc_fb_step(eepacc_handle* h, int B,
                    const double* s, const double* v, const double* v_prev,
                    const double* a_prev, const double* Fm_prev, const double* Fb_prev,
                    const double* t0, const double* s_tv, const double* v_tv,
                    const double* a_tv_prev,
                    double* out, double* s_pred, double* v_pred, int32_t* status,
                    void* stream);
int  eepacc_run_fbmpc(eepacc_handle* h, int B, int n_steps,
                      const double* s0, const double* v0, const double* a_minus1,
                      const double* s_tv, const double* v_tv,
                      double* traj, int32_t* status, void* stream);

/* The same two operators on a handle of eepacc_create_classes: the reference's use cases (GetUseCase.m) or a Settings.m sweep
 * under FBMPC in one launch.  Arguments, layouts and results are those of eepacc_fb_step and eepacc_run_fbmpc (resumption in
 * chunks included); every instance runs with the settings of its class in eepacc_set_classes' map: route tables, W_FB,
 * FBuseTaylor, b_quadr, the estimator modes and time constants, tau_min, h_min, s_goal, N_integratePlant and the whole
 * vehicle.  N_hor and Tvec are class 0's, as for every class handle.  The results of an instance are bit for bit those of
 * eepacc_fb_step / eepacc_run_fbmpc on a handle of eepacc_create from the settings of its class, launched with the same B and
 * n_steps (the kernels are the structured ones, eepacc_fbs.hip, with the class of the instance bound per wave).
 * State.  The entries read and write FBMPC state of the handle's own (warm working set, carried A22 / D2 and predictions,
 * closed-loop carry, step counter) beside the ABMPC state, as on a handle of eepacc_create: eepacc_ab_step / eepacc_run_abmpc
 * and the other ABMPC entries between two of these calls change nothing of their results, and the reverse.  eepacc_reset and
 * eepacc_set_classes reset it.  As with eepacc_run_fbmpc, a closed loop after a step needs eepacc_reset first.
 * eepacc_last_iterations, eepacc_postprocess, eepacc_kpis, eepacc_follow_kpis (EEPACC_FKPI_W_FB) and eepacc_route_kpis work
 * on the result, per class.
 * EEPACC_ENOTSUP, the message naming the entry and the cause: a handle of eepacc_create (use eepacc_fb_step /
 * eepacc_run_fbmpc); a handle of eepacc_create_classes_bl; a class that the structured kernels do not represent (b_quadr(4)
 * != 0, W_FB(1) * b_quadr(5) <= 0, a W_FB outside their signs: the message names the first such class and the field) or a
 * horizon above their LDS budget.  There is no dense path for classes.  EEPACC_EINVAL: a NULL required buffer (s_pred and
 * v_pred may be NULL), B outside [0, max_batch] or different from the last eepacc_set_classes, no map set, n_steps < 0.
 * B = 0 (and n_steps = 0) returns EEPACC_OK.
 * Not built: supplied horizon guesses for FBMPC classes, the condensed QP of an FBMPC step of a class as data
 * (eepacc_classes_build_qp builds the ABMPC problem of such a handle), FBMPC classes through the dense path, and _host and MEX
 * forms of these two entries.
 * Design, code listing and what is measured: DESIGN.md section 3.5f. */
int  eepacc_classes_fb_step(eepacc_handle* h, int B,
                            const double* s, const double* v, const double* v_prev,
                            const double* a_prev, const double* Fm_prev, const double* Fb_prev,
                            const double* t0, const double* s_tv, const double* v_tv,
                            const double* a_tv_prev,
                            double* out, double* s_pred, double* v_pred, int32_t* status,
                            void* stream);
int  eepacc_run_classes_fbmpc(eepacc_handle* h, int B, int n_steps,
                              const double* s0, const double* v0, const double* a_minus1,
                              const double* s_tv, const double* v_tv,
                              double* traj, int32_t* status, void* stream);

/* The condensed QP of one FBMPC step as data, the counterpart of eepacc_ab_build_qp: what a user of the reference holds as H,
 * c, G, g_lb, g_ub after ABO/RunOpt_FBMPC.m:215-264 and finds saved as optSol.H, optSol.G.  The structured FBMPC kernels never
 * form it (they optimise u = Fm + Fb); eepacc_fb_build_qp does, for the inputs of eepacc_fb_step that CreateQP_FB reads
 * (device, each [B]): the estimators and bounds (EstimateVehicleTrajectory.m:55-88, EstimateRouteAndComfortBounds.m:63-171),
 * the objective and rows of ABO/Functions/MPCs/CreateQP_FB.m:158-489, condensed as TransformToDenseFormulation.m:30-91 with
 * the model of RunOpt_FBMPC.m:78-90, 247-259.  Outputs, device, instance-major, in the layout eepacc_qp_solve_batched reads:
 * H [B][nV*nV], g [B][nV], A [B][nV][nC] (column-major nC x nV), lba, uba [B][nC], an absent side -inf / +inf.  There are no
 * lbx / ubx: hand the operator NULL.  H is indefinite.
 * nV = 6 N_hor, variables per stage Fm, Fb, xi_v, xi_h, xi_s, xi_f.  nC = 26 N_hor + 2 plus two rows per blocked stage
 * (Mb[k] = 1, CreateQP_FB.m:346-356), rows in the reference's order (:311-489); eepacc_fb_qp_size returns both.  Covered:
 * both trees, Mb, b_quadr(4) != 0, FBuseTaylor 0 and 1, variable Tvec, every N_hor the handle accepts (the size limit of the
 * dense operator does not apply to the build), the estimator modes 0, 1 and 2 (mode 2 reads the predictions the handle
 * carries from the last FBMPC step).  The slope is the constant one the reference's CreateQP_FB sees (slope(1)).
 *
 * The model A(k), D(k).  With A22 == D2 == NULL the build uses the model the handle's next eepacc_fb_step / eepacc_run_fbmpc
 * step would use: the entries the handle carries and its step counter, with the initialisation at step 0 (:78-90) and the
 * replacement of entry k == step from v_est[N_hor-1] (:247-259); on a handle whose FBMPC steps run through the dense path
 * (Mb, b_quadr(4) != 0, EEPACC_FB_DENSE) B must then be the B of those steps (EEPACC_EINVAL otherwise; ABMPC calls on the
 * handle in between do not matter).  None of it is written back.  The build does not contract products into fused
 * multiply-adds and the step kernels do, so the entry it replaces at k == step can differ from the one the step will compute
 * in the last bit.  With both arrays
 * given ([N_hor][B] each, device) they are the A(k,2,2), D(k,2) the loop holds when it condenses this step; they are used as
 * they are and no step counter is read.  With FBuseTaylor = 0 nothing is carried (A22 = 1, D2 from this step's estimate) and
 * given arrays are EEPACC_EINVAL.  A22_used, D2_used ([N_hor][B] each, device, may be NULL) receive what went into the
 * problem, so that a caller can chain steps without the handle's state.
 *
 * eepacc_fb_qp_rows fills two host arrays [nC]: stage[i] in 0 .. N_hor-1, or N_hor for the two terminal rows, and type[i], one
 * of EEPACC_FB_ROW_*, whose values ascend in the order of the rows within a stage: */
enum {
    EEPACC_FB_ROW_S = 0,       /* CreateQP_FB.m:311-342  s_0 <= s_k <= s_goal                                              */
    EEPACC_FB_ROW_V,           /*   0 <= v_k <= v_max                                                                      */
    EEPACC_FB_ROW_FM,          /*   -1e4 <= Fm_k <= 1e4                                                                    */
    EEPACC_FB_ROW_FB,          /*   -1e4 <= Fb_k <= 0                                                                      */
    EEPACC_FB_ROW_XI_V,        /*   xi_v >= 0                                                                              */
    EEPACC_FB_ROW_XI_H,        /*   xi_h >= 0                                                                              */
    EEPACC_FB_ROW_XI_S,        /*   xi_s >= 0                                                                              */
    EEPACC_FB_ROW_XI_F,        /*   xi_f >= 0                                                                              */
    EEPACC_FB_ROW_BLOCKED_FM,  /* :346-356  Fm_{k-1} - Fm_k = 0, only on a stage with Mb[k] = 1                            */
    EEPACC_FB_ROW_BLOCKED_FB,  /*   Fb_{k-1} - Fb_k = 0, only on a stage with Mb[k] = 1                                    */
    EEPACC_FB_ROW_TM_MIN,      /* :359-366  motor torque  -c v_k + eta_TF/phi Fm_k + xi_f >= -T_m_max                      */
    EEPACC_FB_ROW_TM_MAX,      /*   c v_k + Fm_k/(eta_TF phi) - xi_f <= T_m_max                                            */
    EEPACC_FB_ROW_AXLE_MIN,    /* :369-377  rear-axle traction  (L/mu + h_g) Fm_k + h_g Fb_k + xi_f >= -zeta_w + h_g zeta_rg */
    EEPACC_FB_ROW_AXLE_MAX,    /*   (L/mu - h_g) Fm_k - h_g Fb_k - xi_f <= zeta_w - h_g zeta_rg                            */
    EEPACC_FB_ROW_FRIC_MAX,    /* :380-387  total friction  Fm_k + Fb_k - xi_f <= mu m g cos(theta)                        */
    EEPACC_FB_ROW_FRIC_MIN,    /*   Fm_k + Fb_k + xi_f >= -mu m g cos(theta)                                               */
    EEPACC_FB_ROW_A_MAX,       /* :390-397  Fm_k + Fb_k - xi_f <= lambda m a_max + zeta_a v_est^2 + zeta_rg                */
    EEPACC_FB_ROW_A_MIN,       /*   Fm_k + Fb_k + xi_f >= lambda m a_min + zeta_a v_est^2 + zeta_rg                        */
    EEPACC_FB_ROW_J_MAX,       /* :400-418  (Fm + Fb)_k - (Fm + Fb)_{k-1} - xi_f <= lambda m T_k j_max + ... (stage 0: a_minus1) */
    EEPACC_FB_ROW_J_MIN,       /*   (Fm + Fb)_k - (Fm + Fb)_{k-1} + xi_f >= lambda m T_k j_min + ...                       */
    EEPACC_FB_ROW_V_LIM,       /* :421-442  v_k - xi_f <= speed limit                                                      */
    EEPACC_FB_ROW_V_CURV,      /*   v_k - xi_f <= curve speed                                                              */
    EEPACC_FB_ROW_V_STOP,      /*   v_k - xi_s <= stop speed                                                               */
    EEPACC_FB_ROW_V_TL,        /*   v_k - xi_s <= traffic-light speed                                                      */
    EEPACC_FB_ROW_V_INC,       /* :445-448  speed incentive  v_k + xi_v >= min(speed limit, curve speed)                   */
    EEPACC_FB_ROW_SAFE1,       /* :451-458  safe distance 1  s_k - xi_s <= s_tv - h_min (terminal row :478-489: no slack)  */
    EEPACC_FB_ROW_SAFE2,       /*   safe distance 2  s_k + tau_min v_k - xi_s <= s_tv (terminal row: no slack)             */
    EEPACC_FB_ROW_HWP,         /* :461-473  headway policy, linearised about v_est with FBuseTaylor = 1                    */
    EEPACC_FB_ROW_N
};
/* The built problem is the reference's own: a measured state outside its hard bounds shows up as a stage-0 row without
 * coefficients whose bounds exclude 0.  The constant term of the objective is excluded: 1/2 x'Hx + g'x at the solution equals
 * EEPACC_OUT_COST of the same step, x[0], x[1] are EEPACC_OUT_FM, EEPACC_OUT_FB and x[2..5] are EEPACC_OUT_XI_V, _XI_H,
 * _XI_S, _XI_F (what the extraction of the dense path reads, RunOpt_FBMPC.m:291-299).
 *
 * The build is asynchronous on stream.  Of the handle's state it reads the carried model entries, predictions and step
 * counter named above and nothing else (no warm start, no closed-loop carry), and it writes none: a build between two FBMPC
 * calls leaves their results bit for bit unchanged.  One workgroup per instance writes every entry, zeros included (no
 * memset, no atomics): the arrays do not depend on B or on timing.  EEPACC_EINVAL, with a message that names the argument: a
 * NULL buffer, only one of A22 / D2, B < 0 or B > max_batch.  EEPACC_ENOTSUP: a handle of eepacc_create_classes and a handle
 * created with bl_mode 1 or 2, whose problem eepacc_bl_build_qp builds.  B = 0 returns EEPACC_OK.
 * Throughput: see DESIGN.md section 3.6b (tools/gpu_qp_build_bench.py --family fb times the build against a plain device
 * fill). */
int  eepacc_fb_qp_size(const eepacc_handle* h, int* nV, int* nC);
int  eepacc_fb_qp_rows(const eepacc_handle* h, int32_t* stage, int32_t* type);
int  eepacc_fb_build_qp(eepacc_handle* h, int B,
                        const double* s, const double* v, const double* a_prev, const double* t0,
                        const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        const double* A22, const double* D2,
                        double* H, double* g, double* A, double* lba, double* uba,
                        double* A22_used, double* D2_used, void* stream);

/* FBMPC with the horizon guesses supplied: the contract of CreateQP_FB(OPTsettings, ..., s_est, v_est, s_tv_est, ...)
 * (ABO/RunOpt_FBMPC.m:215), which linearises about v_est (the drag terms of the objective, the acceleration and jerk rows, the
 * headway row with FBuseTaylor = 1), reads the route bounds at s_est, and whose loop makes the model entry A(k), D(k) of MPC
 * step k of v_est(N_hor) (:247-259).  The three entries are the counterparts of eepacc_ab_step_est, eepacc_ab_build_qp_est and
 * eepacc_run_abmpc_preview, above, and the guess arrays follow the same contract:
 *   s_est, v_est, s_tv_est: device arrays [N_hor+1][B], the layout of s_pred / v_pred.
 *   s_est and v_est are given together or both NULL; NULL: the handle's paramEstSetting, mode 2 from the carried predictions
 *   included.  s_tv_est may be NULL: the handle's TVestSetting.  Either side may be given without the other.
 *   Row 0 of s_est and v_est is used as given.  Row N_hor of s_tv_est is not read: the terminal rows use stage N_hor-1
 *   (s_tv_est(N) of CreateQP_FB.m:478-489).  +inf in s_tv_est: no lead at that stage (the three headway rows of the stage, and
 *   the terminal rows if the stage is N_hor-1, then bind nothing).
 *   All three NULL: bit for bit eepacc_fb_step / eepacc_fb_build_qp.
 *   The slope.  The reference's CreateQP_FB sees slope(1) at every stage, whatever s_est says.  eepacc_fb_build_qp_est follows
 *   it, as eepacc_fb_build_qp does.  eepacc_fb_step_est and eepacc_run_fbmpc_preview look the slope up at s_est, as eepacc_fb_step
 *   and eepacc_run_fbmpc do.  On a slope table that is constant (one value along the route) the three agree.  On a table that is
 *   not constant they differ: a supplied s_est then moves the slope of the step, and the step does not solve the problem that
 *   the builder entry writes.  This is the behaviour of the structured FBMPC kernels before these entries and is not tested on
 *   such a table (DESIGN.md sections 3.5e and 7).
 *
 * eepacc_fb_step_est reads and writes exactly the handle state eepacc_fb_step does (working-set codes, the model A22 / D2, the
 * carried predictions, the step counter, the by-step flag): the two can alternate on one handle.  With FBuseTaylor = 1 the
 * entry frozen at k == step is computed from the supplied v_est[N_hor-1]; with FBuseTaylor = 0 D2 comes from the supplied v_est
 * at every stage: what the reference's loop does with those arrays.
 *
 * eepacc_fb_build_qp_est covers what eepacc_fb_build_qp covers (Mb, b_quadr(4) != 0, both FBuseTaylor, dense-path handles, the
 * A22 / D2 rules); it reads no solver state and writes none.  The only difference is where the three guesses come from, and
 * with them the k == step model entry when A22 == D2 == NULL.
 *
 * eepacc_run_fbmpc_preview: eepacc_run_fbmpc with the lead's horizon guess read from the lead trace itself, by exactly the
 * rule of eepacc_run_abmpc_preview: s_tv, v_tv [n_lead][B], n_lead >= n_steps, idx / frac computed once per handle in long
 * double with the same snapping (one table per handle, shared with the ABMPC preview), linear extrapolation past the last row,
 * +inf stays +inf; scenarios.lead_preview states the rule.  The ego estimator stays the handle's.  Launches resume as
 * eepacc_run_fbmpc's do, the caller passing the continued rows.
 *
 * EEPACC_ENOTSUP, the message naming the cause: a handle of eepacc_create_classes / _classes_bl and a handle with bl_mode != 0
 * (all three entries); for the step and the preview entry also a handle whose FBMPC steps go through the dense path (Mb,
 * b_quadr(4) != 0, EEPACC_FB_DENSE=1), where the message says that the builder entry still works.  EEPACC_EINVAL: a NULL
 * required buffer, s_est without v_est or the reverse, B out of range, n_lead < n_steps, and the builder's A22 / D2 rules.
 * B = 0 returns EEPACC_OK.
 * Cost against eepacc_fb_step / eepacc_run_fbmpc: tools/gpu_fb_est_bench.py, DESIGN.md section 3.5e. */
int  eepacc_fb_step_est(eepacc_handle* h, int B,
                        const double* s, const double* v, const double* v_prev,
                        const double* a_prev, const double* Fm_prev, const double* Fb_prev,
                        const double* t0, const double* s_tv, const double* v_tv,
                        const double* a_tv_prev,
                        const double* s_est, const double* v_est, const double* s_tv_est,
                        double* out, double* s_pred, double* v_pred, int32_t* status,
                        void* stream);
int  eepacc_fb_build_qp_est(eepacc_handle* h, int B,
                            const double* s, const double* v, const double* a_prev, const double* t0,
                            const double* s_tv, const double* v_tv, const double* a_tv_prev,
                            const double* s_est, const double* v_est, const double* s_tv_est,
                            const double* A22, const double* D2,
                            double* H, double* g, double* A, double* lba, double* uba,
                            double* A22_used, double* D2_used, void* stream);
int  eepacc_run_fbmpc_preview(eepacc_handle* h, int B, int n_steps, int n_lead,
                              const double* s0, const double* v0, const double* a_minus1,
                              const double* s_tv, const double* v_tv,
                              double* traj, int32_t* status, void* stream);

/* Host-pointer convenience wrappers (what a MEX gateway calls). */
int  eepacc_run_abmpc_host(eepacc_handle* h, int B, int n_steps,
                           const double* s0, const double* v0, const double* a_minus1,
                           const double* s_tv, const double* v_tv,
                           double* traj, int32_t* status);
int  eepacc_run_fbmpc_host(eepacc_handle* h, int B, int n_steps,
                           const double* s0, const double* v0, const double* a_minus1,
                           const double* s_tv, const double* v_tv,
                           double* traj, int32_t* status);

/* Baseline controller by name: optSol = RunOpt_BLMPC(OPTsettings) (ABO/RunOpt_BLMPC.m:1, ABO/Main.m:97) and the body of
 * its loop (:175-300).  Same arguments, outputs and error behaviour as eepacc_ab_step / eepacc_run_abmpc /
 * eepacc_run_abmpc_host; they require a handle created with bl_mode = 1 (EEPACC_EINVAL otherwise), so a binding for
 * RunOpt_BLMPC cannot silently run the ABMPC problem.  The xi_v, xi_h, xi_s entries of the output block are zero
 * (the baseline QP has the one slack xi_f). */
int  eepacc_bl_step(eepacc_handle* h, int B,
                    const double* s, const double* v, const double* a_prev, const double* t0,
                    const double* s_tv, const double* v_tv, const double* a_tv_prev,
                    double* out, double* s_pred, double* v_pred, int32_t* status, void* stream);
int  eepacc_run_blmpc(eepacc_handle* h, int B, int n_steps,
                      const double* s0, const double* v0, const double* a_minus1,
                      const double* s_tv, const double* v_tv,
                      double* traj, int32_t* status, void* stream);
int  eepacc_run_blmpc_host(eepacc_handle* h, int B, int n_steps,
                           const double* s0, const double* v0, const double* a_minus1,
                           const double* s_tv, const double* v_tv,
                           double* traj, int32_t* status);

/* The baseline controller with the horizon guesses supplied: the contract of CreateQP_BL(OPTsettings, n_x, n_u, s_0, v_0, s_est,
 * v_est, s_tv_est, t_0, a_minus1) (ABO/RunOpt_BLMPC.m:56,182), for a handle created with bl_mode = 1.  They are to eepacc_bl_step,
 * eepacc_bl_build_qp and eepacc_run_blmpc what eepacc_ab_step_est, eepacc_ab_build_qp_est and eepacc_run_abmpc_preview are to
 * the ABMPC entries: same arguments, argument order, layouts and NULL rules, so that the yardstick of a use case can be given
 * the lead's future that ABMPC was given.
 * s_est, v_est, s_tv_est: device arrays [N_hor+1][B].  s_est and v_est are given together or both NULL; NULL: the handle's ego
 * estimator.  They reach the problem through the route and comfort bounds alone (EstimateRouteAndComfortBounds,
 * CreateQP_BL.m:46); row 0 is used as given.  s_tv_est may be NULL: the handle's TVestSetting.  It enters only the upper bound
 * of the two safe-distance rows of every stage (CreateQP_BL.m:291,295) and of the two terminal rows, which read s_tv_est(N) of
 * the reference, stage N_hor - 1 here (:309,313): row N_hor is not read.  +inf: no lead at that stage.  With all three NULL the
 * entries compute what eepacc_bl_step / eepacc_bl_build_qp compute, bit for bit.
 * eepacc_bl_step_est reads and writes exactly the handle state eepacc_bl_step does (warm start, the proximal iteration's
 * working set, carried predictions, iteration counts): the two can alternate on one handle.  eepacc_bl_build_qp_est reads no
 * solver state and writes none; eepacc_bl_qp_size and eepacc_bl_qp_rows describe its output.  The problem is a linear program
 * with the reference's weights: compare objective values (EEPACC_OUT_COST), not points.
 * eepacc_run_blmpc_preview: eepacc_run_blmpc with the lead's horizon guess read from the lead trace itself, by the preview rule
 * of eepacc_run_abmpc_preview unchanged (s_tv, v_tv [n_lead][B], n_lead >= n_steps, resumed launches pass the continued rows,
 * past the last row the lead continues at its last speed, +inf stays +inf; scenarios.lead_preview states it in numpy).  The ego
 * estimator stays the handle's.
 * EEPACC_ENOTSUP, the message naming the cause: a handle of eepacc_create_classes / eepacc_create_classes_bl; bl_mode = 0 (the
 * message points to the eepacc_ab_ entries); bl_mode = 2 (the target-vehicle controller has no lead and hands the bounds a
 * zero speed estimate: not built).  EEPACC_EINVAL: a NULL required buffer, s_est without v_est or the reverse, B out of range,
 * n_lead < n_steps.  B = 0 returns EEPACC_OK.
 * Cost against eepacc_bl_step / eepacc_run_blmpc: tools/gpu_bl_est_bench.py, DESIGN.md section 3.7b. */
int  eepacc_bl_step_est(eepacc_handle* h, int B,
                        const double* s, const double* v, const double* a_prev, const double* t0,
                        const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        const double* s_est, const double* v_est, const double* s_tv_est,
                        double* out, double* s_pred, double* v_pred, int32_t* status, void* stream);
int  eepacc_bl_build_qp_est(eepacc_handle* h, int B,
                            const double* s, const double* v, const double* a_prev, const double* t0,
                            const double* s_tv, const double* v_tv, const double* a_tv_prev,
                            const double* s_est, const double* v_est, const double* s_tv_est,
                            double* H, double* g, double* A, double* lba, double* uba, void* stream);
int  eepacc_run_blmpc_preview(eepacc_handle* h, int B, int n_steps, int n_lead,
                              const double* s0, const double* v0, const double* a_minus1,
                              const double* s_tv, const double* v_tv,
                              double* traj, int32_t* status, void* stream);

/* Supplied horizon guesses on a handle with settings classes: eepacc_ab_step_est / eepacc_bl_step_est and
 * eepacc_run_abmpc_preview / eepacc_run_blmpc_preview for the mixed launch, with their arguments, layouts, NULL rules and
 * preview rule unchanged.  The handle decides the controller: one of eepacc_create_classes runs ABMPC (kernels clsest), one of
 * eepacc_create_classes_bl with bl_mode = 1 the baseline controller (kernels blclsest); every instance is solved with the
 * settings of its class in eepacc_set_classes' map, as in eepacc_ab_step / eepacc_run_abmpc on the same handle.  They read and
 * write exactly the handle state those entries do (warm start, carried predictions, closed-loop carry, iteration counts), so
 * they alternate freely with eepacc_ab_step, eepacc_run_abmpc and eepacc_run_blmpc on one handle; a resumed
 * eepacc_run_classes_preview passes the continued rows of the traces.  With s_est, v_est and s_tv_est all NULL
 * eepacc_classes_step_est computes what eepacc_ab_step computes on the handle, bit for bit.  The preview tables are made once
 * per handle from class 0's Tvec, which every class shares.
 * EEPACC_ENOTSUP, the message naming the entry and the cause: a handle without classes (the message points to the plain
 * entries of its mode); a class handle with bl_mode = 2 (no lead).  EEPACC_EINVAL: a call before eepacc_set_classes or with
 * another B than the map's, s_est without v_est or the reverse, n_lead < n_steps, B outside [0, max_batch], a NULL required
 * buffer.  B = 0 returns EEPACC_OK.  The six entries above keep refusing class handles, and so do the plain QP builder
 * entries (eepacc_classes_build_qp, below, builds the problems of a class handle).
 * Cost against twelve launches on plain handles: tools/gpu_classes_est_bench.py, DESIGN.md section 3.4h. */
int  eepacc_classes_step_est(eepacc_handle* h, int B,
                             const double* s, const double* v, const double* a_prev, const double* t0,
                             const double* s_tv, const double* v_tv, const double* a_tv_prev,
                             const double* s_est, const double* v_est, const double* s_tv_est,
                             double* out, double* s_pred, double* v_pred, int32_t* status, void* stream);
int  eepacc_run_classes_preview(eepacc_handle* h, int B, int n_steps, int n_lead,
                                const double* s0, const double* v0, const double* a_minus1,
                                const double* s_tv, const double* v_tv,
                                double* traj, int32_t* status, void* stream);

/* Target-vehicle MPC by name: [s_opt, v_opt, numSolverErrors] = RunOpt_TVMPC(OPTsettings) (ABO/RunOpt_TVMPC.m:1,
 * ABO/Main.m:85) and the body of its loop (:156-277).  They require a handle created with bl_mode = 2 (EEPACC_EINVAL
 * otherwise).  The controller follows no vehicle, so there are no lead inputs.  eepacc_tv_step: device inputs s, v, a_prev,
 * t0 [B]; outputs as eepacc_ab_step.  eepacc_run_tvmpc: n_steps iterations (RunOpt_TVMPC runs t_sim/TV_Ts + 1) from
 * s0 = TVinitDist, v0 = TVinitVel, a_minus1 [B]; t_0 starts at 0 and advances by TV_Ts, the previous solution starts as
 * zeros (:126,134-141); traj [n_steps][EEPACC_OUT_N][B] with EEPACC_OUT_S / EEPACC_OUT_V = s_opt / v_opt and the xi_v,
 * xi_h, xi_s entries zero; status [n_steps][B] mirrors exitMessage (numSolverErrors = its sum).  Like eepacc_run_abmpc a
 * launch continues the previous one until eepacc_reset, so a long trace can be generated in chunks.  The trace can be
 * handed on to eepacc_run_abmpc / _fbmpc / _blmpc of another handle on the device (after subtracting TVlength,
 * ABO/Main.m:88): rows EEPACC_OUT_S and EEPACC_OUT_V of traj are the [n_steps][B] layout those read, with row stride
 * EEPACC_OUT_N * B. */
int  eepacc_tv_step(eepacc_handle* h, int B,
                    const double* s, const double* v, const double* a_prev, const double* t0,
                    double* out, double* s_pred, double* v_pred, int32_t* status, void* stream);
int  eepacc_run_tvmpc(eepacc_handle* h, int B, int n_steps,
                      const double* s0, const double* v0, const double* a_minus1,
                      double* traj, int32_t* status, void* stream);
int  eepacc_run_tvmpc_host(eepacc_handle* h, int B, int n_steps,
                           const double* s0, const double* v0, const double* a_minus1,
                           double* traj, int32_t* status);

/* The condensed QP of one BLMPC or TVMPC step as data, the counterpart of eepacc_ab_build_qp for a handle created with
 * bl_mode = 1 or 2: what a user of the reference holds as H, c, G, g_lb, g_ub and finds saved as optSol.H, optSol.G of a
 * baseline run.  The kernels behind eepacc_bl_step / eepacc_tv_step never form it; eepacc_bl_build_qp does, for the inputs of
 * those entry points (device, each [B]).
 * bl_mode = 1: the problem of ABO/RunOpt_BLMPC.m:182-230 with solverToUse = 1: estimators and bounds
 * (EstimateVehicleTrajectory.m:55-88, EstimateRouteAndComfortBounds.m:63-143,173-189), objective and rows of
 * ABO/Functions/MPCs/CreateQP_BL.m:99-314, condensed as TransformToDenseFormulation.m:30-91.  nV = 2 N_hor, variables per
 * stage a, xi_f; nC = 13 N_hor + 2.
 * bl_mode = 2: the problem of ABO/RunOpt_TVMPC.m:161-208 with ABO/Functions/MPCs/CreateQP_TV.m: the rows of CreateQP_BL
 * without the two safe-distance rows of a stage and without terminal rows, 0.8 of the speed-limit and curve caps
 * (CreateQP_TV.m:265,271) and the comfort limits of a zero speed estimate (:44-45).  nV = 2 N_hor, nC = 11 N_hor.  The lead
 * arguments s_tv, v_tv, a_tv_prev are not read and may be NULL.
 * eepacc_bl_qp_size returns nV and nC of the handle.  Outputs, device, instance-major, in the layout eepacc_qp_solve_batched
 * reads: H [B][nV*nV], g [B][nV], A [B][nV][nC] (column-major nC x nV), lba, uba [B][nC], an absent side -inf / +inf.  There
 * are no lbx / ubx; hand the operator NULL.  Rows are in the reference's order.  The jerk terms take Ts = Tvec[0] at every
 * stage as CreateQP_BL.m:31 does, the dynamics Tvec[k]; the stage-0 jerk rows carry a_minus1 on the right-hand side
 * (:253-261).  H holds the w_a and w_j terms, also where the reference's weights make it zero (a linear program).  Covered:
 * both trees, variable Tvec (bl_mode = 1), every N_hor the handle accepts, the estimator modes 0, 1 and 2 (mode 2 reads the
 * predictions the handle carries from the last step and does not write them), all route features.
 *
 * eepacc_bl_qp_rows fills two host arrays [nC]: stage[i] in 0 .. N_hor-1, or N_hor for the two terminal rows
 * (CreateQP_BL.m:306-314, bl_mode = 1 only), and type[i], one of EEPACC_BL_ROW_*, so that lam_a and ws_a of
 * eepacc_qp_solve_batched_dual on the built problem can be read row by row: which speed-limit, stop or headway row is tight.
 * The values ascend in the order of the rows within a stage; bl_mode = 2 uses the same values and has no SAFE1 / SAFE2 rows: */
enum {
    EEPACC_BL_ROW_S = 0,     /* CreateQP_BL.m:217-228  0 <= s_k <= s_goal                                                  */
    EEPACC_BL_ROW_V,         /*   0 <= v_k <= v_max                                                                        */
    EEPACC_BL_ROW_XI_F,      /*   xi_f >= 0                                                                                */
    EEPACC_BL_ROW_A_MIN,     /* :232-239  a_k + xi_f >= a_min                                                              */
    EEPACC_BL_ROW_A_MAX,     /*   a_k - xi_f <= a_max                                                                      */
    EEPACC_BL_ROW_J_MIN,     /* :242-261  a_k - a_{k-1} + xi_f >= Ts j_min (stage 0: a_minus1 on the right-hand side)      */
    EEPACC_BL_ROW_J_MAX,     /*   a_k - a_{k-1} - xi_f <= Ts j_max                                                         */
    EEPACC_BL_ROW_V_LIM,     /* :265-268  v_k - xi_f <= speed limit (bl_mode = 2: 0.8 of it)                               */
    EEPACC_BL_ROW_V_CURV,    /* :271-274  v_k - xi_f <= curve speed (bl_mode = 2: 0.8 of it)                               */
    EEPACC_BL_ROW_V_STOP,    /* :277-280  v_k - xi_f <= stop speed                                                         */
    EEPACC_BL_ROW_V_TL,      /* :283-286  v_k - xi_f <= traffic-light speed                                                */
    EEPACC_BL_ROW_SAFE1,     /* :289-292  safe distance 1  s_k - xi_f <= s_tv - h_min (terminal row :307-310: no slack)    */
    EEPACC_BL_ROW_SAFE2,     /* :293-296  safe distance 2  s_k + tau_min v_k - xi_f <= s_tv (terminal row :311-314)        */
    EEPACC_BL_ROW_N
};
/* The built problem is the reference's own.  A measured state outside its hard bounds shows up as a stage-0 row without
 * coefficients whose bounds exclude 0; the tolerance state_bound_tol of the kernels is not applied, and neither is their
 * proximal curvature bl_lp_eps.  The constant term of the objective is excluded: 1/2 x'Hx + g'x at a solution equals
 * EEPACC_OUT_COST of the same step.  With the reference's weights the problem is a linear program with faces of optima: compare
 * objective values, not points; x[0] of a solution is an EEPACC_OUT_AQP of the face, x[1] an EEPACC_OUT_XI_F.
 *
 * The build is asynchronous on stream.  It reads no solver state of the handle (warm start, loop counters, carry) and writes
 * none: a build between two eepacc_bl_step / eepacc_run_blmpc / eepacc_tv_step calls leaves their results bit for bit
 * unchanged.  One workgroup per instance writes every entry, zeros included (no memset, no atomics): the arrays do not depend
 * on B or on timing.  EEPACC_EINVAL, with a message that names the argument: a NULL buffer (the lead arrays excepted with
 * bl_mode = 2), B < 0 or B > max_batch.  EEPACC_ENOTSUP: a handle of eepacc_create_classes, and a handle created with
 * bl_mode = 0, whose problems eepacc_ab_build_qp / eepacc_fb_build_qp build.  B = 0 returns EEPACC_OK.
 * Throughput (tools/gpu_qp_build_bench.py --family bl, the build against a plain device fill of the same bytes,
 * profiles/bl_qp_bench.json): 1.34 of the fill's time at N_hor = 20 x 4096 instances, 1.69 at N_hor = 60 x 1024; DESIGN.md
 * section 3.6c. */
int  eepacc_bl_qp_size(const eepacc_handle* h, int* nV, int* nC);
int  eepacc_bl_qp_rows(const eepacc_handle* h, int32_t* stage, int32_t* type);
int  eepacc_bl_build_qp(eepacc_handle* h, int B,
                        const double* s, const double* v, const double* a_prev, const double* t0,
                        const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        double* H, double* g, double* A, double* lba, double* uba, void* stream);

/* The condensed QP of a step as data on a handle with settings classes: eepacc_ab_build_qp(_est) / eepacc_bl_build_qp(_est)
 * for the mixed launch.  One launch writes the problem of every instance with the settings of its class in
 * eepacc_set_classes' map: of a handle of eepacc_create_classes the ABMPC problem (nV = 5 N_hor), of one of
 * eepacc_create_classes_bl the BLMPC or TVMPC problem (nV = 2 N_hor).  These three entries serve class handles only; the
 * nine _qp_size, _qp_rows, _build_qp(_est) entries above keep refusing them.
 *
 * eepacc_classes_qp_size returns nV and nC of the handle.  ABMPC classes may differ in ab_route_rows and so in their row
 * count (14 N_hor + 2 or 18 N_hor + 2; class handles have no Mb); nC is the count of the largest class and the leading row
 * dimension of A, lba and uba for EVERY instance.  The classes of eepacc_create_classes_bl share bl_mode and so the count
 * (13 N_hor + 2 or 11 N_hor).
 * eepacc_classes_qp_rows fills two host arrays [nC] with the row catalogue of class cls: stage[i] and type[i] as
 * eepacc_ab_qp_rows / eepacc_bl_qp_rows give them for a plain handle of that class's settings, in the same order, and behind
 * the class's own rows -1 in both arrays: padding rows.
 * eepacc_classes_build_qp: inputs as eepacc_ab_build_qp_est (device, [B]; s_est, v_est, s_tv_est device [N_hor+1][B] or NULL,
 * s_est and v_est together or both NULL, NULL keeping the estimators of the instance's class).  Outputs, device,
 * instance-major, in the layout eepacc_qp_solve_batched reads: H [B][nV*nV], g [B][nV], A [B][nV][nC] (column-major
 * nC x nV), lba, uba [B][nC].  Over its class's own rows an instance holds, bit for bit, what the plain builder of a handle of
 * that class's settings writes for it; its padding rows hold A exactly 0.0, lba = -inf, uba = +inf, so the dense QP operator
 * takes the arrays as they are and returns padding rows with a zero multiplier and outside the working set.  Every byte of
 * the five arrays is written by the one kernel (no memset, no second pass).  The handle's state is read (estimator mode 2:
 * the carried predictions, as the plain builder), never written.  bl_mode = 2 classes take no lead inputs (s_tv, v_tv,
 * a_tv_prev may be NULL).
 * EEPACC_ENOTSUP, the message naming the entry and the cause: a handle without classes (the message names the plain builder
 * to call); supplied arrays on bl_mode = 2 classes.  EEPACC_EINVAL: a call before eepacc_set_classes or with another B than
 * the map's, B outside [0, max_batch], s_est without v_est or the reverse, a NULL required buffer, cls outside
 * [0, eepacc_num_classes).  B = 0 returns EEPACC_OK.
 * Cost against one plain launch per class and against a device fill: tools/gpu_classes_build_bench.py, DESIGN.md section 3.6d. */
int  eepacc_classes_qp_size(const eepacc_handle* h, int* nV, int* nC);
int  eepacc_classes_qp_rows(const eepacc_handle* h, int cls, int32_t* stage, int32_t* type);
int  eepacc_classes_build_qp(eepacc_handle* h, int B,
                             const double* s, const double* v, const double* a_prev, const double* t0,
                             const double* s_tv, const double* v_tv, const double* a_tv_prev,
                             const double* s_est, const double* v_est, const double* s_tv_est,
                             double* H, double* g, double* A, double* lba, double* uba, void* stream);

/* Post-processing of a closed-loop trajectory (ABO/RunOpt_ABMPC.m:343-349): rpm, Tm,
 * fifth-order battery power P and cumulative energy E, all device [n_steps][B]. */
int  eepacc_postprocess(eepacc_handle* h, int B, int n_steps, const double* traj,
                        double* rpm, double* Tm, double* P, double* E, void* stream);

/* Key figures of a closed-loop run, per instance, on the device: what the reference prints for every run in the report of
 * ABO/Main.m:131-263 and the fuel economy of ABO/Custom_plots.m:73-107.  Inputs, device: traj [n_steps][EEPACC_OUT_N][B] and
 * status [n_steps][B] as every eepacc_run_* entry point writes them; rows S, V, FM and A of traj are read, the other eight
 * are not.  Output, device: kpi [EEPACC_KPI_N][B], batch-major, raw SI units without rounding (km, kWh and the
 * 0.1*round(10 t) of the travel time are left to the caller).  cutoff_dist_host, host, [the handle's number of classes]:
 * cutOffDist of every class, `cut` below; it may be reused when the call returns.  With n = n_steps, Ts = Tvec[0],
 * P_k the fifth-order surface b_fifthOrder at (Fm_k, 30/pi v_k phi) (ABO/RunOpt_ABMPC.m:343-349, as eepacc_postprocess)
 * and E_k = Ts sum_{i<=k} P_i: */
enum {
    EEPACC_KPI_BAD_EXITS = 0,    /* Main.m:210  count of status != 0 over all steps                                       */
    EEPACC_KPI_DISTANCE_M,       /* Main.m:220  s[n-1]                                                                    */
    EEPACC_KPI_ENERGY_J,         /* Main.m:226  E[n-1]                                                                    */
    EEPACC_KPI_CUTOFF_INDEX,     /* Main.m:150-161  ind: the first i >= 1 with s[i-1] < cut < s[i], else n-1 (0-based i;  */
                                 /*             the reference's 1-based index of the sample before)                       */
    EEPACC_KPI_REACHED,          /* 1.0 if such an i exists, else 0.0                                                     */
    EEPACC_KPI_VLIM_ERR,         /* Main.m:133,232  InterpPWA(cut, s_speedLim, v_speedLim) - v[ind-2]                     */
    EEPACC_KPI_ENERGY_CUTOFF_J,  /* Main.m:245  E[ind-2]                                                                  */
    EEPACC_KPI_TIME_CUTOFF_S,    /* Main.m:238  ind * Ts                                                                  */
    EEPACC_KPI_A_MAX,            /* Main.m:257  max, min and root mean square of a[0 .. ind-1]                            */
    EEPACC_KPI_A_MIN,
    EEPACC_KPI_A_RMS,
    EEPACC_KPI_J_MAX,            /* Main.m:261  the same of j[0 .. ind-1], j[k] = (a[k+1] - a[k]) / Ts (n-1 entries)      */
    EEPACC_KPI_J_MIN,
    EEPACC_KPI_J_RMS,
    EEPACC_KPI_FUEL_KG,          /* Custom_plots.m:81-90  Ts/1000 sum_{k>=1} FC_k, FC = max(0.25, p00 + p10 v + p01 TW),  */
                                 /*             TW = max(0, (lambda m a + F0 + F2 v^2) R_w); the first sample counts zero */
    EEPACC_KPI_FE_L_PER_100KM,   /* Custom_plots.m:100-107  FUEL_KG / 0.835 / (max_k s[k] / 1000) * 100                   */
    EEPACC_KPI_N
};
/* Two cases the reference leaves open are fixed here.  Where ind < 2 the sample index ind-2 is taken as 0 (MATLAB would
 * stop with an index error, a 0-based host port wraps to the last sample).  Where n_steps = 1 there is no jerk and no
 * sample before the cut-off: ind = 0, the three jerk figures are 0 and the acceleration figures are those of a[0].
 *
 * Works on every kind of handle (ABMPC in all variants, BLMPC, TVMPC, FBMPC); on a handle of eepacc_create_classes every
 * instance is evaluated with the constants and the cut-off of its class (eepacc_set_classes must have been called for
 * this B).  Asynchronous on stream; reads and writes no carried state of the handle, and a result does not depend on
 * timing: the same input gives the same bits.  EEPACC_EINVAL, with a message that names the argument: a NULL buffer,
 * n_steps < 1, B > max_batch, a class map that is not set or was set for another B, a cut-off that is not finite.
 * B = 0 returns EEPACC_OK.
 *
 * Launch geometry, for callers who choose sizes: a workgroup of EEPACC_KPI_WAVES waves serves 64 instances and each
 * wave reduces max(EEPACC_KPI_MIN_SLICE, ceil(n_steps / EEPACC_KPI_WAVES)) consecutive steps. */
#define EEPACC_KPI_WAVES      16
#define EEPACC_KPI_MIN_SLICE   8
int  eepacc_kpis(eepacc_handle* h, int B, int n_steps, const double* traj, const int32_t* status,
                 const double* cutoff_dist_host, double* kpi, void* stream);

/* Vehicle-following and cost key figures of a closed-loop run, per instance, on the device: how the ego kept its distance
 * to the lead (the headway distance s_tv - s_opt and headway time (s_tv - s_opt)./v_opt of ABO/Main.m:679-771 against the
 * minimum-headway policy max(h_min, v tau_min) of :687) and what every term of the objective cost over the run (the last
 * entries of the cumulative series cost_a .. cost_xi_f of ABO/RunOpt_ABMPC.m:382-404 and cost_P of
 * ABO/RunOpt_FBMPC.m:373-397, which Main.m:1043-1151 plots).  Inputs, device: traj [n_steps][EEPACC_OUT_N][B] and status
 * [n_steps][B] as every eepacc_run_* entry point writes them, s_tv and v_tv [n_steps][B] as it reads them.  Rows S, V, A,
 * XI_V, XI_H, XI_S, XI_F of traj are read, row FM where the weight of COST_P is not zero; status is not read.  Output,
 * device: fkpi [EEPACC_FKPI_N][B], batch-major, raw SI units.  With n = n_steps, Ts = Tvec[0], the gap h_k = s_tv[k] - s[k],
 * the jerk j_k = (a[k+1] - a[k]) / Ts, and a "lead sample" a k with s_tv[k] < 1e6 (the reference's "no lead" is a lead
 * at 1e6 m or more, Main.m:288; a NaN is no lead sample): */
enum {
    EEPACC_FKPI_LEAD_SAMPLES = 0,  /* number of lead samples                                                              */
    EEPACC_FKPI_H_MIN_M,           /* min h_k over the lead samples; +inf if there is none                                */
    EEPACC_FKPI_H_MIN_INDEX,       /* the first k that attains it; -1.0 if there is none                                  */
    EEPACC_FKPI_THW_MIN_S,         /* Main.m:752-764  min h_k / v_k over the lead samples with v_k > 0; +inf if none      */
    EEPACC_FKPI_MARGIN_MIN_M,      /* Main.m:687  min (h_k - max(h_min, v_k tau_min)) over the lead samples; +inf if none */
    EEPACC_FKPI_MARGIN_VIOL_STEPS, /* number of lead samples with that margin < 0                                         */
    EEPACC_FKPI_TTC_MIN_S,         /* time to collision: min h_k / (v_k - v_tv[k]) over the lead samples with             */
                                   /* v_k - v_tv[k] > 0; +inf if none.  Not in the reference.                             */
    EEPACC_FKPI_XI_H_MAX,          /* max_k xi_h[k] over all n steps                                                      */
    EEPACC_FKPI_COST_P,            /* RunOpt_FBMPC.m:383  w_P sum_{k<=n-2} P_k^2, P_k the fifth-order surface of          */
                                   /* eepacc_kpis; 0 where w_P = 0, without evaluating the surface                        */
    EEPACC_FKPI_COST_A,            /* RunOpt_ABMPC.m:392  w_a sum_{k<=n-2} a_k^2                                          */
    EEPACC_FKPI_COST_J,            /* :393  w_j sum_{k<=n-2} j_k^2, all n-1 jerks                                         */
    EEPACC_FKPI_COST_XI_V,         /* :394  w_v sum_{k<=n-2} xi_v[k]                                                      */
    EEPACC_FKPI_COST_XI_H,         /* :395  w_h sum_{k<=n-2} xi_h[k]                                                      */
    EEPACC_FKPI_COST_XI_S,         /* :396  w_s sum_{k<=n-2} xi_s[k]                                                      */
    EEPACC_FKPI_COST_XI_F,         /* :397  w_f sum_{k<=n-2} xi_f[k]                                                      */
    EEPACC_FKPI_N
};
/* The cost sums run over k = 1:N_sim of the reference, N_sim = n - 1: the last sample is in none of them, and n_steps = 1
 * gives seven zeros.  The minima, the maximum and the index come from comparisons alone (`<`, `>`; the first of equal gaps
 * wins), v_k tau_min, h_k / v_k and a_k a_k are each rounded once: these fields and the two counts are exact.
 *
 * A handle of eepacc_create serves eepacc_run_abmpc and eepacc_run_fbmpc alike, so `weights` says whose weights apply: */
enum {
    EEPACC_FKPI_W_AB = 0,   /* W(1..5) of RunOpt_ABMPC.m:383-388 for w_a, w_j, w_v, w_h, w_s and w_f = W(5) again; COST_P = 0.   */
                            /* W is OPTsettings.W_AB as the reference's user wrote it: with ab_fuel_term = 0 (ORIG, six entries, */
                            /* stored here behind a leading 0) that is W_AB[1..5] of eepacc_settings, otherwise (ABO, seven      */
                            /* entries) W_AB[0..4], where W(1) is w_FC -- the reference's cost_a uses it all the same, so does   */
                            /* this                                                                                              */
    EEPACC_FKPI_W_FB,       /* W_FB[0..6] = w_P, w_a, w_j, w_v, w_h, w_s, w_f (RunOpt_FBMPC.m:373-379)                           */
    EEPACC_FKPI_W_NONE      /* all weights 1: the raw sums, and COST_P = 0 (RunOpt_BLMPC and RunOpt_TVMPC define no cost_*)      */
};
/* Works on every kind of handle; h_min, tau_min, the weights and the power surface come from a table of the operator's own
 * with one entry per class, built at creation.  On a handle of eepacc_create_classes every instance is evaluated with the
 * constants of its class (eepacc_set_classes must have been called for this B).  Asynchronous on stream; reads and writes
 * no carried state of the handle.  The geometry is that of eepacc_kpis (EEPACC_KPI_WAVES, EEPACC_KPI_MIN_SLICE), the
 * slices are joined by one wave in slice order without atomics: a result depends on n_steps and on nothing else, not on B,
 * not on timing, not on the kind of handle.  EEPACC_EINVAL, with a message that names the argument: another value of
 * weights, n_steps < 1, a NULL buffer, B < 0 or B > max_batch, a class map that is not set or was set for another B.
 * B = 0 returns EEPACC_OK.  Throughput: not measured. */
int  eepacc_follow_kpis(eepacc_handle* h, int B, int n_steps, int weights, const double* traj, const int32_t* status,
                        const double* s_tv, const double* v_tv, double* fkpi, void* stream);

/* Route-compliance key figures of a closed-loop run, per instance, on the device: whether the ego obeyed its route -- the
 * sign-posted speed limit, the curve speed, the stop-sign profile and the red lights, which the reference shows only as
 * pictures of one run (speed over distance, ABO/Main.m:374-433; distance over time against the red phases, :486-534) -- and
 * whether it stayed inside the comfort envelope of EstimateRouteAndComfortBounds.m:154-189.  It judges what the plant did:
 * the slacks xi_s, xi_f of traj say what the QP planned.  Inputs, device: traj [n_steps][EEPACC_OUT_N][B] and status
 * [n_steps][B] as every eepacc_run_* entry point writes them; rows S, V and A of traj are read; status is not read (it is
 * kept for symmetry with eepacc_kpis and eepacc_follow_kpis and must not be NULL).  t_start: the time of row 0, 0 for a run
 * from eepacc_reset and k0 Ts for the rows of a resumed launch.  tol_host [3], host: v_tol, a_tol, j_tol, finite and >= 0;
 * it may be reused when the call returns.  Outputs, device: rkpi [EEPACC_RKPI_N][B], batch-major, raw SI units; limits
 * [n_steps][EEPACC_RLIM_N][B], or NULL: the four caps below at every sample, for redrawing the two figures per instance. */
enum {
    EEPACC_RLIM_V_LIM = 0,   /* the sign-posted speed limit at s_k */
    EEPACC_RLIM_V_CURV,      /* the curve speed at s_k             */
    EEPACC_RLIM_V_STOP,      /* the stop-sign profile at s_k       */
    EEPACC_RLIM_V_TL,        /* the red-light cap at s_k, t_k      */
    EEPACC_RLIM_N
};
/* With n = n_steps, Ts = Tvec[0] and t_k = t_start + k Ts (one rounded product, one rounded sum), the caps at sample k are
 * these.  The table judges a run and is not bug-compatible with the planner: every deviation from the controller's own
 * look-up, EstimateRouteAndComfortBounds.m (line numbers below; route_bounds of csrc/eepacc_stage.h restates it), is named.
 *   v_lim   v_speedLim[j] on s_speedLim[j] <= s < s_speedLim[j+1]; v_speedLim[0] before the first knot (and for a NaN),
 *           v_speedLim[last] from the last knot on.  Deviation: :93 takes the position s_speedLim(end) as the limit there.
 *   v_curv  alpha_TTL |curvature[j]|^(-1/3) on the same half-open intervals of s_curv, first and last held outside.
 *           Deviation: :107 has open intervals and falls through to the last entry for a position exactly on a knot.
 *   v_stop  min_j (|stopLoc_j - s| stopRefVelSlope + stopVel), the profile of Main.m:375-385; 1e5 without stops.
 *           Deviation: :116-123 applies the term within stopRefDist only and lets the last stop in range win.
 *   v_TL    the minimum, over the lights j that are red at t_k and have |TLLoc_j - s| < stopRefDist, of the three-branch cap
 *           of :133-139; 1e5 if there is none.  Light j is red at t when mod(t - TLLoc(j,2), TLLoc(j,3) + TLLoc(j,4)) <
 *           TLLoc(j,3), mod being MATLAB's (a cycle of length 0 returns its argument).  Deviations: the phase is taken at the
 *           sample's own time, not at the t_0 + i Tvec(i) of :130; of several lights the lowest cap counts, not the last.
 *   comfort a_min, a_max, j_min, j_max at v_k from :154-172; on a handle created with bl_mode != 0 the baseline branch
 *           :173-189 with the handle's BL_*_Lim* (a NaN speed takes the branch of v >= 20).  j_k = (a[k+1] - a[k]) / Ts, k <= n-2. */
enum {
    EEPACC_RKPI_VLIM_EXCESS_MAX = 0,     /* max_k (v_k - v_lim_k)                                                            */
    EEPACC_RKPI_VLIM_EXCESS_INDEX,       /* the first k that attains it; -1.0 if no sample could be taken (all NaN)          */
    EEPACC_RKPI_VLIM_VIOL_STEPS,         /* number of k with v_k - v_lim_k > v_tol                                           */
    EEPACC_RKPI_VCURV_EXCESS_MAX,        /* the same against v_curv                                                          */
    EEPACC_RKPI_VCURV_VIOL_STEPS,
    EEPACC_RKPI_VSTOP_EXCESS_MAX,        /* the same against v_stop                                                          */
    EEPACC_RKPI_VSTOP_VIOL_STEPS,
    EEPACC_RKPI_VTL_EXCESS_MAX,          /* the same against v_TL, over the samples with v_TL < 1e5 only; -inf and 0 if none */
    EEPACC_RKPI_VTL_VIOL_STEPS,
    EEPACC_RKPI_STOPS_PASSED,            /* number of pairs (k >= 1, stop j) with s[k-1] < stopLoc_j <= s[k]                 */
    EEPACC_RKPI_STOP_CROSS_V_MAX,        /* max over them of min(v[k-1], v[k]); -inf if there is none                        */
    EEPACC_RKPI_TL_PASSED,               /* number of pairs (k >= 1, light j) with s[k-1] < TLLoc_j <= s[k]                  */
    EEPACC_RKPI_RED_CROSSINGS,           /* those with the light red at t_{k-1} and at t_k                                   */
    EEPACC_RKPI_RED_CROSSINGS_POSSIBLE,  /* those with the light red at t_{k-1} or at t_k                                    */
    EEPACC_RKPI_RED_CROSS_FIRST_INDEX,   /* the first k of the latter; -1.0 if there is none                                 */
    EEPACC_RKPI_A_OVER_MAX,              /* max_k (a_k - a_max(v_k))                                                         */
    EEPACC_RKPI_A_UNDER_MAX,             /* max_k (a_min(v_k) - a_k)                                                         */
    EEPACC_RKPI_J_OVER_MAX,              /* max_{k<=n-2} (j_k - j_max(v_k)); -inf at n = 1                                   */
    EEPACC_RKPI_J_UNDER_MAX,             /* max_{k<=n-2} (j_min(v_k) - j_k); -inf at n = 1                                   */
    EEPACC_RKPI_COMFORT_VIOL_STEPS,      /* number of k with an acceleration excess > a_tol or a jerk excess > j_tol         */
    EEPACC_RKPI_V_MIN,                   /* min_k v_k (a measured speed can fall below zero)            */
    EEPACC_RKPI_N
};
/* Exactness: every figure is a maximum, a minimum, a count or an index, and there are no sums.  Maxima and the minimum are
 * kept by `>` and `<` from -inf and +inf, so where values are equal the first one wins, within a slice and across slices, and
 * a NaN is never taken and never counted.  Every product, sum and quotient is rounded once (contraction is off for the unit).
 * All fields, and limits, therefore equal the numpy specification report.route_table / report.route_limits bit for bit.
 *
 * Limit: a stop line or light crossed between the last row of one call and the first row of the next is seen by neither call,
 * and neither is the jerk between those two rows.  A run made in chunks concatenates its rows first.
 *
 * Works on every kind of handle; the route tables, the five stop / light constants and the baseline limits come from a table
 * of the operator's own with one entry per class, built at creation.  On a handle of eepacc_create_classes every instance is
 * judged on the route of its class (eepacc_set_classes must have been called for this B).  Asynchronous on stream; reads and
 * writes no carried state of the handle.  The geometry is that of eepacc_kpis (EEPACC_KPI_WAVES, EEPACC_KPI_MIN_SLICE): a line
 * crossed between k-1 and k belongs to the slice that holds k, limits is written by the slice that owns the sample, and the
 * slices are joined by one wave in slice order without atomics, so a result depends on n_steps and the inputs only, not on B,
 * the instance's position, timing or the kind of handle.  EEPACC_EINVAL, with a message that names the argument: a NULL
 * traj, status, tol_host or rkpi, n_steps < 1, B < 0 or B > max_batch, a tolerance that is negative or not finite, t_start not
 * finite, a class map that is not set or was set for another B.  B = 0 returns EEPACC_OK.  Throughput: not measured. */
int  eepacc_route_kpis(eepacc_handle* h, int B, int n_steps, double t_start, const double* tol_host,
                       const double* traj, const int32_t* status, double* rkpi, double* limits, void* stream);

/* Solver statistics of the last launch, device [B]: active-set iterations used. */
int  eepacc_last_iterations(eepacc_handle* h, int B, int32_t* iters_host);

/* Wait for the work queued on `stream` and report the handle's sticky device error word:
 * EEPACC_EDEVICE if a closed-loop launch since the last eepacc_reset could not hand its loop state
 * on (affected steps carry status 3), EEPACC_OK otherwise.  The *_host wrappers call it themselves. */
int  eepacc_synchronize(eepacc_handle* h, void* stream);

/* Flag string the library was compiled with ("" for a release build; instrumented builds such as
 * -DEEPACC_AB_TIMING change the meaning of the iteration / status outputs). */
const char* eepacc_build_flags(void);

#ifdef __cplusplus
}
#endif
#endif /* EEPACC_H */
