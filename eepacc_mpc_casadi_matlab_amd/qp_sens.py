"""Derivatives of the dense QP operator's solution on its final working set.

    min 1/2 x'Hx + g'x   s.t.  lba <= Ax <= uba,  lbx <= x <= ubx

With (x, lam_a, lam_x, ws_a, ws_x) from ``Engine.qp_solve_batched_dual`` (CasADi's sign: Hs x + g + A'lam_a + lam_x = 0,
Hs = (H+H')/2) the solution satisfies, on the rows and variables the working set holds,

    Hs x + A_W' lam_a + E_W' lam_x = -g,     A_i x = (bound held),     x_j = (bound held).

While the working set stays what it is this is a linear system in (x, lam), and differentiating it gives

    K [dx; dlam] = [-(dg + dHs x + dA' lam_a);  d(bound held) - dA x;  d(bound held)],    K = [Hs N'; N 0]

with N the held rows of A and unit rows of the held variables.  ``Engine.qp_kkt_solve`` (eepacc_qp_kkt_solve_batched)
solves with K on the device.  K is symmetric, so for a scalar loss L with gradients (gx, glam) the same solve
[u; w] = K^-1 [gx; glam] gives dL = u' r_p + w' r_c, i.e.

    dL/dg = -u,   dL/d(bound held) = w,   dL/dH = -(u x' + x u')/2,   dL/dA = -(lam_a u' + w_a x').

The result is the derivative of the QP's solution where strict complementarity holds.  A held row with lam == 0 is
treated as held: the result is then the derivative on that working set, a one-sided derivative of the solution.

``kkt_solve_reference`` is the numpy specification of the device entry; ``jvp_rhs`` and ``vjp_grads`` are the two recipes
as plain array arithmetic (numpy arrays or torch tensors, leading batch axis), so they run without an engine.
"""
from __future__ import annotations

import numpy as np

LD = np.longdouble


# ------------------------------------------------------------------------------------------- numpy specification
def kkt_matrix(H, A, ws_a, ws_x):
    """(K, rows, vars): the full KKT matrix [Hs N'; N 0] of one problem in float64, the indices of the held rows of A and
    of the held variables (codes +-1; anything else is not held)."""
    H = np.asarray(H, dtype=np.float64); n = H.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, n); m = A.shape[0]
    wa = np.zeros(m, dtype=int) if ws_a is None else np.asarray(ws_a).reshape(m).astype(int)
    wx = np.zeros(n, dtype=int) if ws_x is None else np.asarray(ws_x).reshape(n).astype(int)
    rows = np.nonzero(np.abs(wa) == 1)[0]; cols = np.nonzero(np.abs(wx) == 1)[0]
    k = len(rows) + len(cols)
    N = np.zeros((k, n))
    N[:len(rows)] = A[rows]
    N[len(rows) + np.arange(len(cols)), cols] = 1.0
    K = np.zeros((n + k, n + k))
    K[:n, :n] = 0.5 * (H + H.T)
    K[n:, :n] = N; K[:n, n:] = N.T
    return K, rows, cols


def _gauss_solve(K, rhs):
    """K^-1 rhs in numpy.longdouble: Gaussian elimination with partial pivoting on [K | rhs], then refinement against
    long-double residuals until the correction stops shrinking.  Raises LinAlgError on a zero pivot."""
    N = K.shape[0]
    Kl = K.astype(LD)
    M = Kl.copy()
    perm = np.arange(N)
    for k in range(N):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        if M[p, k] == 0:
            raise np.linalg.LinAlgError("singular KKT matrix")
        if p != k:
            M[[k, p]] = M[[p, k]]; perm[[k, p]] = perm[[p, k]]
        M[k + 1:, k] /= M[k, k]
        M[k + 1:, k + 1:] -= np.outer(M[k + 1:, k], M[k, k + 1:])

    def solve(b):
        y = b[perm].copy()
        for k in range(N):
            y[k + 1:] -= M[k + 1:, k][:, None] * y[k]
        for k in range(N - 1, -1, -1):
            y[k] /= M[k, k]
            y[:k] -= M[:k, k][:, None] * y[k]
        return y

    b = rhs.astype(LD)
    z = solve(b)
    last = np.inf
    for _ in range(10):
        dz = solve(b - Kl @ z)
        step = float(np.abs(dz).max(initial=0.0))
        if not step < 0.5 * last:
            break
        z = z + dz
        last = step
    return z


def kkt_solve_reference(H, A, ws_a, ws_x, r_p, r_a=None, r_x=None):
    """Specification of eepacc_qp_kkt_solve_batched for ONE problem: the full KKT matrix of the working set, no
    elimination, solved in numpy.longdouble.  r_p [nV] or [nR,nV]; r_a [.., nC], r_x [.., nV] or None (zeros).
    Returns (p, q_a, q_x, resid) shaped like the right-hand sides (float64; q is 0.0 outside the working set) and
    resid = the scaled inf-norm residual of the returned float64 values (kkt_residual)."""
    K, rows, cols = kkt_matrix(H, A, ws_a, ws_x)
    n = np.asarray(H).shape[0]; m = np.asarray(A).reshape(-1, n).shape[0]
    r_p = np.asarray(r_p, dtype=np.float64)
    flat = r_p.ndim == 1
    rp = r_p.reshape(-1, n); nR = rp.shape[0]
    ra = np.zeros((nR, m)) if r_a is None else np.asarray(r_a, dtype=np.float64).reshape(nR, m)
    rx = np.zeros((nR, n)) if r_x is None else np.asarray(r_x, dtype=np.float64).reshape(nR, n)
    rhs = np.concatenate([rp, ra[:, rows], rx[:, cols]], axis=1).T          # [n + k, nR]
    z = _gauss_solve(K, rhs)
    p = np.asarray(z[:n].T, dtype=np.float64)
    q_a = np.zeros((nR, m)); q_x = np.zeros((nR, n))
    q_a[:, rows] = np.asarray(z[n:n + len(rows)].T, dtype=np.float64)
    q_x[:, cols] = np.asarray(z[n + len(rows):].T, dtype=np.float64)
    resid = kkt_residual(H, A, ws_a, ws_x, rp, ra, rx, p, q_a, q_x)
    if flat:
        return p[0], q_a[0], q_x[0], resid
    return p, q_a, q_x, resid


def kkt_residual(H, A, ws_a, ws_x, r_p, r_a, r_x, p, q_a, q_x):
    """Scaled inf-norm residual of the stated system, evaluated in numpy.longdouble from the problem data:
    max |K z - r| / max(1, |r|_inf, |K|_max |z|_inf), the largest over the right-hand sides."""
    K, rows, cols = kkt_matrix(H, A, ws_a, ws_x)
    n = np.asarray(H).shape[0]; m = np.asarray(A).reshape(-1, n).shape[0]
    rp = np.asarray(r_p, dtype=np.float64).reshape(-1, n); nR = rp.shape[0]
    ra = np.zeros((nR, m)) if r_a is None else np.asarray(r_a, dtype=np.float64).reshape(nR, m)
    rx = np.zeros((nR, n)) if r_x is None else np.asarray(r_x, dtype=np.float64).reshape(nR, n)
    p = np.asarray(p, dtype=np.float64).reshape(nR, n)
    qa = np.asarray(q_a, dtype=np.float64).reshape(nR, m); qx = np.asarray(q_x, dtype=np.float64).reshape(nR, n)
    rhs = np.concatenate([rp, ra[:, rows], rx[:, cols]], axis=1).T.astype(LD)
    z = np.concatenate([p, qa[:, rows], qx[:, cols]], axis=1).T.astype(LD)
    res = K.astype(LD) @ z - rhs
    kmax = np.abs(K).max(initial=0.0)
    worst = 0.0
    for r in range(nR):
        den = max(1.0, float(np.abs(rhs[:, r]).max(initial=0.0)), float(kmax * np.abs(z[:, r]).max(initial=0.0)))
        worst = max(worst, float(np.abs(res[:, r]).max(initial=0.0)) / den)
    return worst


# ------------------------------------------------------------------ the two recipes (numpy arrays or torch tensors)
def _col(M, v):
    return (M @ v[..., None])[..., 0]


def jvp_rhs(x, lam_a, ws_a, ws_x, dg=None, dlba=None, duba=None, dlbx=None, dubx=None, dH=None, dA=None):
    """Right-hand sides (r_p, r_a, r_x) of the forward derivative, all arrays with a leading batch axis:
    r_p = -(dg + dHs x + dA' lam_a), r_a = d(bound of the held side) - dA x on held rows, r_x = d(bound of the held side).
    A direction that is None is zero."""
    r_p = 0.0 * x
    r_a = 0.0 * lam_a
    r_x = 0.0 * x
    if dg is not None:
        r_p = r_p - dg
    if dH is not None:
        r_p = r_p - 0.5 * _col(dH + dH.swapaxes(-1, -2), x)
    if dA is not None:
        r_p = r_p - _col(dA.swapaxes(-1, -2), lam_a)
        r_a = r_a - (ws_a != 0) * _col(dA, x)
    if dlba is not None:
        r_a = r_a + (ws_a == -1) * dlba
    if duba is not None:
        r_a = r_a + (ws_a == 1) * duba
    if dlbx is not None:
        r_x = r_x + (ws_x == -1) * dlbx
    if dubx is not None:
        r_x = r_x + (ws_x == 1) * dubx
    return r_p, r_a, r_x


def vjp_grads(x, lam_a, ws_a, ws_x, u, w_a, w_x):
    """Gradients of a scalar loss from the adjoint solve (u, w_a, w_x) = K^-1 (gx, glam_a, glam_x), leading batch axis:
    dict with g [B,nV], lba, uba [B,nC], lbx, ubx [B,nV], H [B,nV,nV] and A_cm [B,nV,nC] -- dL/dA in the operator's
    column-major layout; A_cm.swapaxes(1, 2) is dL/dA as [B,nC,nV]."""
    return dict(g=-u,
                lba=(ws_a == -1) * w_a, uba=(ws_a == 1) * w_a,
                lbx=(ws_x == -1) * w_x, ubx=(ws_x == 1) * w_x,
                H=-0.5 * (u[..., :, None] * x[..., None, :] + x[..., :, None] * u[..., None, :]),
                A_cm=-(u[..., :, None] * lam_a[..., None, :] + x[..., :, None] * w_a[..., None, :]))


# ---------------------------------------------------------------------------------------------------- on the device
def _dev(eng, v, dtype=None):
    t = eng.torch
    return None if v is None else t.as_tensor(v, dtype=dtype or t.float64, device=eng.device)


def qp_jvp(eng, sol, H, A, dg=None, dlba=None, duba=None, dlbx=None, dubx=None, dH=None, dA=None):
    """Directional derivative of the solution `sol` (a QpDualResult of eng.qp_solve_batched_dual for H [B,nV,nV],
    A [B,nC,nV]) along the data directions given (None: zero): returns (dx, dlam_a, dlam_x, status) as device tensors.
    status [B] is the linear solve's (1: singular working set, outputs NaN).  The working set is taken as fixed; a held
    row with lam == 0 counts as held (one-sided derivative)."""
    d = [_dev(eng, v) for v in (dg, dlba, duba, dlbx, dubx, dH, dA)]
    r_p, r_a, r_x = jvp_rhs(sol.x, sol.lam_a, sol.ws_a, sol.ws_x, *d)
    return eng.qp_kkt_solve(H, A, sol.ws_a, sol.ws_x, r_p, r_a, r_x)


def qp_vjp(eng, sol, H, A, gx, glam_a=None, glam_x=None):
    """Gradients of a scalar loss with respect to all data of the QP, from its gradients gx [B,nV], glam_a [B,nC],
    glam_x [B,nV] (None: zero) with respect to the solution: the dict of vjp_grads plus A = dL/dA as [B,nC,nV] (a view
    of A_cm) and status [B].  One adjoint solve on the device; the outer products are torch operations there.
    Instances with sol.status != 0, or a singular working set, get NaN."""
    t = eng.torch
    p, q_a, q_x, st = eng.qp_kkt_solve(H, A, sol.ws_a, sol.ws_x, _dev(eng, gx), _dev(eng, glam_a), _dev(eng, glam_x))
    gr = vjp_grads(sol.x, sol.lam_a, sol.ws_a, sol.ws_x, p, q_a, q_x)
    bad = (sol.status != 0) | (st != 0)
    for k, v in gr.items():
        gr[k] = t.where(bad.reshape((-1,) + (1,) * (v.dim() - 1)), t.full_like(v, float("nan")), v)
    gr["A"] = gr["A_cm"].transpose(1, 2)
    gr["status"] = st
    return gr


def lead_gradient_from_uba(g_uba, stage, typ, N):
    """dL/ds_tv_est [B, N+1] from dL/duba [B, nC] of a problem of Engine.ab_build_qp / ab_build_qp_est and its row table
    (stage, typ) of Engine.ab_qp_rows.  The lead's guess enters that problem only through uba of the rows safe1, safe2 and
    hwp, each with coefficient 1 (CreateQP_AB.m:355-371), so entry k is the sum of g_uba over those rows of stage k.  The
    two terminal rows (stage N in the table) read s_tv_est(N) of the reference, row N - 1 of the array, and are credited
    there; row N of the array is not read and gets 0.  numpy arrays or torch tensors."""
    from ._abi import AB_ROW
    stage = np.asarray(stage).reshape(-1); typ = np.asarray(typ).reshape(-1)
    lead = (typ == AB_ROW["safe1"]) | (typ == AB_ROW["safe2"]) | (typ == AB_ROW["hwp"])
    sel = np.zeros((stage.size, N + 1))
    sel[np.nonzero(lead)[0], np.minimum(stage[lead], N - 1)] = 1.0
    if isinstance(g_uba, np.ndarray):
        return g_uba @ sel
    return g_uba @ g_uba.new_tensor(sel)


def ab_lead_gradient(eng, qp, sol, rows, gx, solver=None):
    """Gradient of a scalar loss on the solution x of an ABMPC step with respect to the lead prediction s_tv_est: [B, N+1]
    (device tensor; row N_hor of s_tv_est is not read, its entry is 0).  qp: the AbQp of eng.ab_build_qp_est (or
    ab_build_qp), sol: the QpDualResult of eng.qp_solve_batched_dual on it, rows: eng.ab_qp_rows(), gx [B, nV]: dL/dx
    (x[0] is the applied acceleration EEPACC_OUT_AQP).  One adjoint solve (qp_vjp), then lead_gradient_from_uba.  Exactly 0
    for a stage none of whose lead rows is in the working set; NaN where qp_vjp gives NaN.
    On an engine of from_classes with ABMPC classes qp is the AbQp of eng.classes_build_qp and rows is not read (None will do):
    every instance is summed over the lead rows of the catalogue of its own class (eng.classes_qp_rows), so the mix of a
    launch is differentiated in one adjoint solve; padding rows have no type and contribute nothing.  solver: the engine
    whose dense QP operator solved the problem and runs the adjoint solve (default eng); a class engine has no dense operator
    of its own, so any ordinary Engine on the same device is named here."""
    gr = qp_vjp(solver if solver is not None else eng, sol, qp.H, qp.A, gx)
    class_of = getattr(eng, "class_of", None)
    if class_of is None:
        return lead_gradient_from_uba(gr["uba"], rows[0], rows[1], eng.N)
    if qp.H.shape[1] != 5 * eng.N:
        raise ValueError("ab_lead_gradient differentiates the ABMPC problem; the classes of this engine are baseline or target-vehicle settings")
    g_uba = gr["uba"]
    out = g_uba.new_zeros((g_uba.shape[0], eng.N + 1))
    for c in np.unique(class_of):
        idx = eng.torch.as_tensor(np.nonzero(class_of == c)[0], device=g_uba.device)
        stage, typ = eng.classes_qp_rows(int(c))
        out[idx] = lead_gradient_from_uba(g_uba[idx], stage, typ, eng.N)
    return out


_FUNCTION = None


def _function(torch):
    global _FUNCTION
    if _FUNCTION is not None:
        return _FUNCTION

    class QPFunction(torch.autograd.Function):
        """forward: eng.qp_solve_batched_dual; backward: qp_vjp.  Inputs (eng, H, g, A, lba, uba, lbx, ubx), bounds may be
        None; outputs (x, lam_a, lam_x, status).  See qp_layer."""

        @staticmethod
        def forward(ctx, eng, H, g, A, lba, uba, lbx, ubx):
            sol = eng.qp_solve_batched_dual(H, g, A, lba, uba, lbx, ubx)
            ctx.eng = eng
            # the outputs go through save_for_backward: kept on ctx directly they would close a reference cycle
            # (output -> grad_fn -> ctx -> output) that holds device memory until the garbage collector runs
            ctx.save_for_backward(H, A, sol.x, sol.lam_a, sol.lam_x, sol.ws_a, sol.ws_x, sol.status)
            ctx.mark_non_differentiable(sol.status)
            return sol.x, sol.lam_a, sol.lam_x, sol.status

        @staticmethod
        def backward(ctx, gx, glam_a, glam_x, _gstatus):
            from .engine import QpDualResult
            H, A, x, lam_a, lam_x, ws_a, ws_x, status = ctx.saved_tensors
            sol = QpDualResult(x=x, cost=None, status=status, lam_a=lam_a, lam_x=lam_x, ws_a=ws_a, ws_x=ws_x, iters=None)
            # lam is identically zero outside the working set, and NaN gradients of a failed instance's NaN outputs
            # must not reach the solve of the others: the solve reads glam on held entries only
            gr = qp_vjp(ctx.eng, sol, H, A, gx, glam_a, glam_x)
            need = ctx.needs_input_grad
            out = [None, gr["H"], gr["g"], gr["A"], gr["lba"], gr["uba"], gr["lbx"], gr["ubx"]]
            return tuple(v if need[i] else None for i, v in enumerate(out))

    _FUNCTION = QPFunction
    return QPFunction


def __getattr__(name):
    if name == "QPFunction":                       # torch is imported only when the autograd layer is asked for
        import torch
        return _function(torch)
    raise AttributeError(name)


def qp_layer(eng, H, g, A, lba=None, uba=None, lbx=None, ubx=None):
    """Differentiable QP layer: (x, lam_a, lam_x, status) = QPFunction.apply(eng, H, g, A, lba, uba, lbx, ubx) for float64
    tensors on the engine's device, H [B,nV,nV], g [B,nV], A [B,nC,nV], bounds [B,nC] / [B,nV] or None.
    The forward pass is eng.qp_solve_batched_dual, the backward pass one adjoint solve on the final working set
    (qp_vjp).  Instances with status != 0 get NaN gradients.  A held row with lam == 0 is treated as held: the gradient is
    then the derivative on that working set, which is a one-sided derivative of the solution; across a change of the
    working set the solution is not differentiable and nothing here says so."""
    return _function(eng.torch).apply(eng, H, g, A, lba, uba, lbx, ubx)
