"""What the GPU suites of the three condensed-QP builders (test_gpu_ab_build.py, test_gpu_fb_build.py, test_gpu_bl_build.py)
set up alike."""
import numpy as np

INS = ("s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev")      # the [B] inputs of a _build_qp, in argument order


def _engine(OPT, V, max_batch=128):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


def _cols(inps):
    """A list of per-instance input dicts as one array per input."""
    return {n: np.array([float(d[n]) for d in inps]) for n in INS}


def _np(q):
    return [x.cpu().numpy() for x in q]
