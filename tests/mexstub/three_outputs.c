/*
 * three_outputs.c -- adapter between tests/mexstub/mex_mock.c, which calls mexFunction for ONE output struct, and a gateway
 * with the call form [a, b, c] = f(OPTsettings): the gateway is compiled with -DmexFunction=gateway_mexFunction, called
 * here with nlhs = 3 as MATLAB would, and its outputs are packed into a struct with the fields out1, out2, out3.
 */
#include "mex.h"

void gateway_mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
    mxArray* out[3] = {0, 0, 0};
    mxArray* S = mxCreateStructMatrix(1, 1, 0, 0);
    (void)nlhs;
    gateway_mexFunction(3, out, nrhs, prhs);
    mxSetField(S, 0, "out1", out[0]);
    mxSetField(S, 0, "out2", out[1]);
    mxSetField(S, 0, "out3", out[2]);
    plhs[0] = S;
}
