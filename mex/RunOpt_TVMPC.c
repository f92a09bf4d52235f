/*
 * RunOpt_TVMPC.c -- MEX gateway: [s_opt, v_opt, numSolverErrors] = RunOpt_TVMPC(OPTsettings)
 *                                                                   (ABO/RunOpt_TVMPC.m:1, ABO/Main.m:85)
 * Drop-in for the target-vehicle MPC's closed loop, the controller that generates the lead vehicle's trace along the
 * route; see eepacc_mex_common.h for the contract and the build line
 *     mex -I../include RunOpt_TVMPC.c -L../eepacc_mpc_casadi_matlab_amd -leepacc
 * The target-vehicle MPC is a handle created with bl_mode = 2, run through eepacc_run_tvmpc_host (include/eepacc.h):
 * horizon TV_N_hor with the uniform step TV_Ts (RunOpt_TVMPC.m:18,20), estimator TV_trajEstSett
 * (EstimateVehicleTrajectory.m:20-24), weights W_TV (CreateQP_TV.m:27,36-39), comfort limits TV_*_Lim*Vel
 * (EstimateRouteAndComfortBounds.m:47-52), start TVinitDist / TVinitVel / a_minus1 (RunOpt_TVMPC.m:22-24).  No lead trace
 * is read.  RunPlantModel.m steps the plant by Tvec(1): TV_Ts must equal it, anything else is refused.
 */
#define EEPACC_MEX_NO_LEAD
#include "eepacc_mex_common.h"

static eepacc_handle* g_handle = NULL;
static void at_exit(void) { if (g_handle) { eepacc_destroy(g_handle); g_handle = NULL; } }

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    if (nrhs != 1 || !mxIsStruct(prhs[0]) || nlhs > 3)
        mexErrMsgIdAndTxt("eepacc:usage", "usage: [s_opt, v_opt, numSolverErrors] = RunOpt_TVMPC(OPTsettings)");
    const mxArray* O = prhs[0];
    (void)emx_build_optsol;                         /* the optSol struct of the ego controllers: not what RunOpt_TVMPC returns */
    eepacc_mex_inputs in;
    emx_read_inputs(O, 0, &in);                     /* everything the controllers share (W_AB is read but not used) */
    eepacc_settings* S = &in.S;
    int n;
    /* the target-vehicle MPC's own view of the settings, carried in the baseline controller's fields */
    S->bl_mode = 2;
    const double Ts = emx_scalar(O, "TV_Ts");                                   /* RunOpt_TVMPC.m:20 */
    if (Ts != in.Ts) mexErrMsgIdAndTxt("eepacc:badField", "TV_Ts must equal Tvec(1), the step of the plant model (RunPlantModel.m)");
    S->N_hor = (int)emx_scalar(O, "TV_N_hor");                                  /* :18 */
    if (S->N_hor < 2 || S->N_hor > EEPACC_MAX_HORIZON) mexErrMsgIdAndTxt("eepacc:badField", "TV_N_hor must be in [2, %d]", EEPACC_MAX_HORIZON);
    double* Tv = (double*)mxMalloc(sizeof(double) * (size_t)S->N_hor);
    for (int i = 0; i < S->N_hor; ++i) Tv[i] = Ts;
    S->Tvec = Tv;
    mxFree(in.Mb);
    in.Mb = (int32_t*)mxCalloc((size_t)S->N_hor, sizeof(int32_t));              /* no move blocking in RunOpt_TVMPC */
    S->Mb = in.Mb;
    S->paramEstSetting = (int)emx_scalar(O, "TV_trajEstSett");                  /* EstimateVehicleTrajectory.m:22 */
    {
        const double* W = emx_vector(O, "W_TV", &n, 1);                         /* CreateQP_TV.m:27,36-39 */
        if (n != 4) mexErrMsgIdAndTxt("eepacc:badField", "W_TV must have 4 entries [w_v, w_a, w_j, w_f]");
        memcpy(S->W_BL, W, sizeof(double) * 4);
    }
    S->BL_a_LimLowVel = emx_scalar(O, "TV_a_LimLowVel"); S->BL_a_LimHighVel = emx_scalar(O, "TV_a_LimHighVel");
    S->BL_j_LimLowVel = emx_scalar(O, "TV_j_LimLowVel"); S->BL_j_LimHighVel = emx_scalar(O, "TV_j_LimHighVel");
    S->bl_lp_eps = 0.0; S->state_bound_tol = 0.0;                               /* library defaults */
    const double s0 = emx_scalar(O, "TVinitDist"), v0 = emx_scalar(O, "TVinitVel");     /* :22-23 */
    at_exit();
    mexAtExit(at_exit);
    if (eepacc_create(&g_handle, S, &in.V, 0, 1) != EEPACC_OK)
        mexErrMsgIdAndTxt("eepacc:create", "%s", eepacc_last_error());
    const int ns = in.n_steps;                                                  /* kk = 0:N_sim, :129 */
    double* traj = (double*)mxMalloc(sizeof(double) * (size_t)ns * EEPACC_OUT_N);
    int32_t* status = (int32_t*)mxMalloc(sizeof(int32_t) * (size_t)ns);
    const int rc = eepacc_run_tvmpc_host(g_handle, 1, ns, &s0, &v0, &in.a_minus1, traj, status);
    at_exit();
    if (rc != EEPACC_OK) mexErrMsgIdAndTxt("eepacc:run", "%s", eepacc_last_error());
    mxArray* s_opt = emx_col(ns);
    mxArray* v_opt = emx_col(ns);
    double nerr = 0.0;                                                          /* numSolverErrors = sum(exitMessage), :280 */
    for (int k = 0; k < ns; ++k) {
        mxGetPr(s_opt)[k] = traj[(size_t)k * EEPACC_OUT_N + EEPACC_OUT_S];
        mxGetPr(v_opt)[k] = traj[(size_t)k * EEPACC_OUT_N + EEPACC_OUT_V];
        nerr += status[k] != 0;
    }
    plhs[0] = s_opt;
    if (nlhs > 1) plhs[1] = v_opt; else mxDestroyArray(v_opt);
    if (nlhs > 2) plhs[2] = mxCreateDoubleScalar(nerr);
    mxFree(traj); mxFree(status); mxFree(in.Mb); mxFree(Tv); if (in.TLLoc) mxFree(in.TLLoc);
}
